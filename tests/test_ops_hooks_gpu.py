"""The two launch hooks of dge_amd.ops (PROFILE: bench.py's roofline pass; KERNEL_LOG: which kernels ran on which stream) on each of
the four conv-family launchers: a hooked launch computes the same bits as a plain one and leaves exactly the entries the readers
expect - (start event, stop event, algorithmic flops, tag, algorithmic bytes) and (kernel name, stream handle)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _nbytes(*ts):
    return sum(t.numel() * t.element_size() for t in ts)


def _conv2d(ops, g):
    B, H, W, cin, cout, k = 1, 16, 16, 32, 32, 3
    x = torch.randn(B, H, W, cin, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randn(cout, cin, k, k, device=DEV, generator=g)
    wp = ops.pack_conv_weight(w, ops.pack_mode_for(w, ops.PACK_FWD, H, W, ops.BF16), ops.BF16, 1.0 / math.sqrt(k * k * cin))
    run = lambda: ops.conv2d(x, wp, cout, k, act=ops.ACT_LRELU, gain=math.sqrt(2.0))
    return run, 2 * k * k * cin * cout * H * W * B, lambda y: _nbytes(x, y, wp), 0


def _conv_pp(ops, g):
    B, H, W, cin, cout = 12, 33, 97, 96, 256            # tests/test_conv_pp_gpu.py: test_ragged_shapes
    assert ops.conv_pp_supported(B, H, W, cin, cout, ops.BF16)
    x = torch.randn(B, H, W, cin, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randn(cout, cin, 3, 3, device=DEV, generator=g)
    s = 1.0 + 0.3 * torch.randn(B, cin, device=DEV, generator=g)
    d = 0.5 + torch.rand(B, cout, device=DEV, generator=g)
    wpp = ops.pack_conv_pp(w, 1.0 / math.sqrt(9 * cin), in_scale=s, out_scale=d, gain=math.sqrt(2.0))
    bias = 0.2 * torch.randn(cout, device=DEV, generator=g)
    run = lambda: ops.conv_pp(x, wpp, cout, bias=bias, act=ops.ACT_LRELU, gain=math.sqrt(2.0))
    return run, 2 * 9 * cin * cout * H * W * B, lambda y: _nbytes(x, y, wpp), 1


def _up_pp(ops, g):
    cin, cout, H, W, B = 160, 32, 17, 45, 3             # tests/test_fullsize_gpu.py: UP_PP_LAYERS
    assert ops.up_pp_supported(B, H, W, cin, cout, ops.BF16)
    x = torch.randn(B, H, W, cin, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randn(cout, cin, 3, 3, device=DEV, generator=g)
    s = 1.0 + 0.3 * torch.randn(B, cin, device=DEV, generator=g)
    d = 0.5 + torch.rand(B, cout, device=DEV, generator=g)
    wimg = ops.pack_up_pp(ops.pack_upconv_weight(w, ops.BF16, 1.0 / math.sqrt(9 * cin)), cout, cin, in_scale=s, out_scale=d, gain=math.sqrt(2.0))
    bias = 0.2 * torch.randn(cout, device=DEV, generator=g)
    run = lambda: ops.up_pp(x, wimg, cout, bias=bias, act=ops.ACT_LRELU, gain=math.sqrt(2.0))
    # (the weight images are counted by formula: 9*Cin*Cout bf16 values per sample)
    return run, 2 * 9 * cin * cout * H * W * B, lambda y: _nbytes(x, y) + 18 * cin * cout * B, 1


def _upconv_fir(ops, g):
    B, H, W, cin, cout = 2, 8, 8, 32, 32                # tests/test_upconv_gpu.py, f32
    assert ops.upconv_supported(cin, cout, ops.F32)
    x = torch.randn(B, H, W, cin, device=DEV, generator=g)
    w = torch.randn(cout, cin, 3, 3, device=DEV, generator=g)
    s = 1.0 + 0.3 * torch.randn(B, cin, device=DEV, generator=g)
    d = 0.5 + torch.rand(B, cout, device=DEV, generator=g)
    wu = ops.pack_upconv_weight(w, ops.F32, 1.0 / math.sqrt(9 * cin))
    run = lambda: ops.upconv_fir(x, wu, cout, in_scale=s, out_scale=d, act=ops.ACT_LRELU, gain=math.sqrt(2.0))
    return run, 2 * 9 * cin * cout * H * W * B, lambda y: _nbytes(x, y, wu), 0


@pytest.mark.parametrize("case", [_conv2d, _conv_pp, _up_pp, _upconv_fir], ids=lambda f: f.__name__[1:])
def test_hooked_launch_is_bit_equal_and_leaves_its_entries(case):
    from dge_amd import ops
    run, flops, nbytes, logged = case(ops, torch.Generator(device=DEV).manual_seed(77))
    assert ops.PROFILE is None and ops.KERNEL_LOG is None
    y0 = run()
    prof, log = [], []
    ops.PROFILE, ops.KERNEL_LOG = prof, log
    try:
        y1 = run()
    finally:
        ops.PROFILE, ops.KERNEL_LOG = None, None
    torch.cuda.synchronize()
    assert y1.shape == y0.shape and torch.equal(y0, y1)
    assert len(prof) == 1 and len(prof[0]) == 5
    e0, e1, fl, tag, nb = prof[0]
    assert fl == flops and isinstance(fl, float)
    assert nb == nbytes(y1)
    assert isinstance(tag, tuple) and tag[0] == y0.shape[0]
    assert len(log) == logged
    for name, stream in log:
        assert isinstance(name, str) and name and stream.value == ops._stream().value
    assert e0.elapsed_time(e1) >= 0
