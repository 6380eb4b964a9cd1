"""ops.up_dgrad_stream (csrc/upconv_stream_bwd.hip): the data gradient of the 64 -> 32 up layer as one streaming launch - FIR^T, the
9-tap adjoint of the transposed conv on the t grid (stylegan2_generator.py:879-896 differentiated) and the data-gradient epilogue,
with or without the tail backward of the layer below (:908-921 differentiated) - against oracle/conv_ref.py (adjoint of up_linear)
and oracle/elem_ref.py (autograd of the tail), the construction of test_fullsize_gpu.py::
test_data_gradient_with_fused_tail_backward_fullsize, on the smallest shapes at which the kernel's structure can go wrong; and the
synthesis backward of a small generator whose top up layer takes the new route."""
import functools
import math

import pytest
import torch

from tests.conftest import golden
from tests.golden import recipe as R
from tests.helpers import s2_shapes
from oracle import conv_ref as CR
from oracle import elem_ref as ER

pytestmark = pytest.mark.gpu
DEV = "cuda"
CIN, COUT = 64, 32               # of the forward layer
GAIN, NS = math.sqrt(2.0), 0.37


def _act(B, H, W, C, g, scale=1.0):
    return (torch.randn(B, H, W, C, device=DEV, generator=g) * scale).to(torch.bfloat16)


def _nchw(x_nhwc, b):
    return x_nhwc[b:b + 1].float().permute(0, 3, 1, 2).contiguous().cpu()


def _one_rounding(got, ref, slack=1e-5):
    """largest violation of |got - ref| <= 2^-8 |ref| + slack*max|ref| (<= 0 means every element is within one bf16 rounding)"""
    return ((got - ref).abs() - (2.0 ** -8) * ref.abs() - slack * ref.abs().max()).max().item()


def _relmax(got, ref):
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def _up_dgrad(g, w, H, W):
    """CR.up_dgrad for a rectangular input grid (the oracle's own body: autograd of CR.up_linear)"""
    x = torch.zeros(g.shape[0], w.shape[1], H, W, requires_grad=True)
    return torch.autograd.grad(CR.up_linear(x, w, 1.0), x, g)[0]


SHAPES = [(2, 20, 20),        # one strip narrower than 32
          (2, 37, 70),        # three strips, ragged last strip, odd row count (uneven row segments)
          (1, 64, 64),        # exact strips
          (2, 128, 128)]      # several row segments per strip


@functools.lru_cache(maxsize=None)
def _case(B, H, W, with_add):
    """inputs on the device and the CPU reference of every sample, computed once per (shape, addend) and left unchanged"""
    g = torch.Generator(device=DEV).manual_seed(15000 + 7 * H + W + (1 if with_add else 0))
    gz_in = _act(B, 2 * H, 2 * W, COUT, g)
    d_in = 0.5 + torch.rand(B, COUT, device=DEV, generator=g)            # per-sample factors that differ between the samples
    xin = _act(B, H, W, CIN, g, 1.5)                                      # stored output of the layer below
    add = _act(B, H, W, CIN, g) if with_add else None
    w = torch.randn(COUT, CIN, 3, 3, device=DEV, generator=g).to(torch.bfloat16).float()
    wscale = 1.0 / math.sqrt(9 * CIN)
    s = 1.0 + 0.3 * torch.randn(B, CIN, device=DEV, generator=g)
    noise = torch.randn(1, H, W, device=DEV, generator=g)
    wq = CR.bf16_round(w.cpu() * wscale)
    ref = []
    for b in range(B):
        gy = _nchw(gz_in, b) * d_in[b].cpu()[None, :, None, None]
        raw = CR.up_dgrad(gy, wq, 1.0, H) if H == W else _up_dgrad(gy, wq, H, W)
        gref = raw * s[b].cpu()[None, :, None, None]
        if with_add:
            gref = gref + _nchw(add, b)
        xb = _nchw(xin, b)
        ref_gz, ref_R = ER.modconv_tail_bwd(xb, gref, torch.ones(CIN), noise[0].cpu(), GAIN)
        rd, xd, gzd = raw.double(), xb.double(), ref_gz.double()
        zt = ER.lrelu_inverse(xd, GAIN) - NS * noise[0].cpu().double()[None, None]
        ref.append(dict(g=gref, gz=ref_gz,
                        dot=(rd * xd).sum((0, 2, 3)), dot_abs=(rd * xd).abs().sum((0, 2, 3)),
                        acc=rd.sum((0, 2, 3)), acc_abs=rd.abs().sum((0, 2, 3)),
                        P=torch.stack([ref_R[:, 0] - NS * ref_R[:, 1], ref_R[:, 2]], 1),
                        P_abs=torch.stack([(gzd * zt).abs().sum((0, 2, 3)), gzd.abs().sum((0, 2, 3))], 1)))
    return dict(gz_in=gz_in, d_in=d_in, xin=xin, add=add, w=w, wscale=wscale, s=s, noise=noise, ref=ref)


def test_support_predicate():
    from dge_amd import ops
    assert ops.up_dgrad_stream_supported(8, 512, 512, 64, 32, ops.BF16)
    assert ops.up_dgrad_stream_supported(1, 20, 20, 64, 32, ops.BF16)
    assert not ops.up_dgrad_stream_supported(8, 512, 512, 64, 32, ops.F32)
    assert not ops.up_dgrad_stream_supported(8, 256, 256, 128, 64, ops.BF16)
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        assert not ops.up_dgrad_stream_supported(8, 512, 512, 64, 32, ops.BF16)
    finally:
        ops.set_deterministic(was)


@pytest.mark.nondet
@pytest.mark.parametrize("with_prep", [False, True])
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_up_dgrad_stream_vs_oracle(B, H, W, with_add, with_prep):
    """Every sample and every pixel (all four image borders: that is where the FIR^T padding and the out-of-range DMA lanes act).
    Bounds: the ones the project holds this layer's current launches to (test_fullsize_gpu.py) - values within one bf16 rounding
    with slack 6e-3 of the maximum (g_t = FIR^T(g_z) * d is rounded to bf16 once before the MFMAs: one operand
    rounding), without prep also 7.5e-3 of the maximum; dot statistics 8e-4 (Hin <= 64) / 9e-5 of the sum of |terms|; prep
    sums 7.9e-3 of the sum of |terms|."""
    from dge_amd import ops
    from dge_amd._lib import last_kernel
    c = _case(B, H, W, with_add)
    wp = ops.pack_up_dgrad_stream(c["w"], ops.BF16, c["wscale"])
    st = ops.SlotStats(B, CIN, DEV)
    P = ops.SlotStats(B, CIN, DEV)
    prep = dict(gain=GAIN, noise=c["noise"], ns=torch.tensor([NS], device=DEV), stats=P) if with_prep else None
    out = ops.up_dgrad_stream(c["gz_in"], wp, c["d_in"], c["s"], c["add"], st, c["xin"], prep=prep)
    assert last_kernel() == "upconv_stream_bwd<bf16,64,32>" + ("+prep" if with_prep else "")
    assert tuple(out.shape) == (B, H, W, CIN)
    stc = st.buf.sum(0).cpu().double()
    dot_bound = 8e-4 if H <= 64 else 9e-5
    for b in range(B):
        r = c["ref"][b]
        got = _nchw(out, b)
        want = r["gz"] if with_prep else r["g"]
        viol = _one_rounding(got, want.float(), slack=6e-3)
        e_dot = ((stc[b, :, 0] - r["dot"]).abs() / r["dot_abs"]).max().item()
        print(f"MEAS up_dgrad_stream {(B, H, W)} add={with_add} prep={with_prep} b={b} rounding_viol={viol:.3e} "
              f"relmax={_relmax(got, want.float()):.3e} dot={e_dot:.3e}", end="")
        assert viol <= 0, (b, viol)
        assert e_dot < dot_bound, (b, e_dot)
        if with_prep:
            Pt = P.buf.sum(0).cpu().double()
            e_p = ((Pt[b] - r["P"]).abs() / r["P_abs"]).max().item()
            print(f" prep={e_p:.3e}")
            assert e_p < 7.9e-3, (b, e_p)
        else:
            e_acc = ((stc[b, :, 1] - r["acc"]).abs() / r["acc_abs"]).max().item()
            print(f" acc={e_acc:.3e}")
            assert _relmax(got, want.float()) < 7.5e-3, b
            assert e_acc < dot_bound, (b, e_acc)


@pytest.mark.nondet
def test_synthesis_backward_takes_the_streaming_route_for_its_top_up_layer(monkeypatch):
    """The 64^2 generator of tests/golden/s2_small.npz: its top up layer (layer 7, 32^2 -> 64^2) is 64 -> 32 channels.  g_wp of the
    synthesis backward in the default (atomics) mode with the switch on and off against the reference's autograd gradient, bound of
    test_s2_gpu.py::test_synthesis_grad_wp_vs_reference_golden (bf16: 8e-2); with the switch on the tail backward of layer 6 rides
    the new launch (no modconv_bwd_prep pass) and layer 6's style gradient leaves through s2_style_grads."""
    import numpy as np
    import dge_amd
    from dge_amd import ops, s2_conv
    assert not ops.is_deterministic()
    g = golden("s2_small.npz")
    Pm = R.fill_s2(s2_shapes(64, fmaps_base=2048, fmaps_max=128), seed=11)
    G = dge_amd.StyleGAN2Generator(64, fmaps_base=2048, fmaps_max=128, compute_dtype="bf16").cuda()
    G.load_state_dict(Pm)
    L7 = G.synthesis.layer7
    assert L7.up and (L7.in_c, L7.out_c, L7.res) == (64, 32, 64)
    assert ops.up_dgrad_stream_supported(2, 32, 32, L7.in_c, L7.out_c, ops.BF16)
    want = torch.as_tensor(np.asarray(g["grad_wp"])).float()
    calls = {}
    real_prep, real_sg, real_up = ops.modconv_bwd_prep, ops.s2_style_grads, ops.up_dgrad_stream
    errs = {}
    for on in (True, False):
        monkeypatch.setattr(s2_conv, "UP_DG_STREAM", on)
        seen = dict(prep_shapes=[], rows=[], kernels=[])
        calls[on] = seen

        def spy_prep(g_x, *a, _s=seen, **k):
            _s["prep_shapes"].append(tuple(g_x.shape))
            return real_prep(g_x, *a, **k)

        def spy_sg(blocks, *a, _s=seen, **k):
            _s["rows"] += [b["row"] for b in blocks if "P" in b]
            return real_sg(blocks, *a, **k)

        def spy_up(*a, _s=seen, **k):
            out = real_up(*a, **k)
            _s["kernels"].append(dge_amd._lib.last_kernel())
            return out

        monkeypatch.setattr(ops, "modconv_bwd_prep", spy_prep)
        monkeypatch.setattr(ops, "s2_style_grads", spy_sg)
        monkeypatch.setattr(ops, "up_dgrad_stream", spy_up)
        wp = R.randn("s2.wp", (2, 10, 512), 5).cuda().requires_grad_(True)
        img = G.synthesis(wp)["image"]
        gimg = R.randn("s2.gimg", tuple(img.shape), 5, 1.0 / img.numel() ** 0.5).cuda()
        (img * gimg).sum().backward()
        errs[on] = ((wp.grad.float().cpu() - want).abs().max() / want.abs().max()).item()
    print(f"MEAS grad_wp stream on {errs[True]:.3e} off {errs[False]:.3e}")
    assert errs[True] < 8e-2 and errs[False] < 8e-2, errs
    assert calls[True]["kernels"] == ["upconv_stream_bwd<bf16,64,32>+prep"] and calls[False]["kernels"] == []
    # (with the switch off this layer's 32^2 input grid takes the phase form of conv_igemm, which carries the tail backward too; the
    #  512^2 grid of the 1024^2 generator does not - s2_conv.dgrad_takes_prep)
    assert (2, 32, 32, 64) not in calls[True]["prep_shapes"] and 6 in calls[True]["rows"], calls[True]
