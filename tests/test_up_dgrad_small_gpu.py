"""ops.up_dgrad_small (csrc/conv_small.hip, phase flavour): the data gradient of the low-resolution 256 / 512-channel up layers as
ops.fir_t2d + the 9 non-zero (phase, offset) units on the low-resolution kernel - the adjoint of the transposed conv on the t grid
(stylegan2_generator.py:879-896 differentiated) with the data-gradient epilogue, with or without the tail backward of the layer
below (:908-921 differentiated) - against oracle/conv_ref.py (adjoint of up_linear) and oracle/elem_ref.py (autograd of the tail),
the construction of test_up_dgrad_stream_gpu.py; against the launch it replaces (ops.conv2d(in_t2d=True)); its packed weight copy;
and the synthesis backward of a small generator with 512-channel low layers, whose three up layers take the new route."""
import functools
import math

import pytest
import torch

from tests.golden import recipe as R
from tests.helpers import s2_shapes
from oracle import conv_ref as CR
from oracle import elem_ref as ER
from oracle import ref_torch as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
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


# (C = out channels of the forward layer = K of a unit, N = its in channels, B, H, W of the input grid, noise per sample)
SHAPES = [(256, 64, 2, 8, 8, False),        # the smallest the kernel takes
          (512, 128, 2, 4, 4, True),        # one tile, a quarter of it image
          (512, 128, 2, 8, 8, False),       # exact tile
          (512, 128, 1, 12, 20, True),      # ragged, non-square, several tiles
          (512, 128, 2, 16, 16, False),
          (512, 512, 3, 32, 32, True)]      # 384 workgroups: more than the compute units, a workgroup slot runs twice
IDS = ["%d-%d-%dx%dx%d" % s[:5] for s in SHAPES]


@functools.lru_cache(maxsize=None)
def _case(C, N, B, H, W, per_sample_noise, with_add):
    """inputs on the device and the CPU reference of every sample, computed once per (shape, addend) and left unchanged"""
    g = torch.Generator(device=DEV).manual_seed(17000 + 7 * H + W + C + N + (1 if with_add else 0))
    gz_in = _act(B, 2 * H, 2 * W, C, g)
    d_in = 0.5 + torch.rand(B, C, device=DEV, generator=g)               # per-sample factors that differ between the samples
    xin = _act(B, H, W, N, g, 1.5)                                        # stored output of the layer below
    add = _act(B, H, W, N, g) if with_add else None
    w = torch.randn(C, N, 3, 3, device=DEV, generator=g).to(torch.bfloat16).float()
    wscale = 1.0 / math.sqrt(9 * N)
    s = 1.0 + 0.3 * torch.randn(B, N, device=DEV, generator=g)
    noise = torch.randn(B if per_sample_noise else 1, H, W, device=DEV, generator=g)
    wq = CR.bf16_round(w.cpu() * wscale)
    ref = []
    for b in range(B):
        nz = noise[b if per_sample_noise else 0].cpu()
        gy = _nchw(gz_in, b) * d_in[b].cpu()[None, :, None, None]
        raw = CR.up_dgrad(gy, wq, 1.0, H) if H == W else _up_dgrad(gy, wq, H, W)
        gref = raw * s[b].cpu()[None, :, None, None]
        if with_add:
            gref = gref + _nchw(add, b)
        xb = _nchw(xin, b)
        ref_gz, ref_R = ER.modconv_tail_bwd(xb, gref, torch.ones(N), nz, GAIN)
        rd, xd, gzd = raw.double(), xb.double(), ref_gz.double()
        zt = ER.lrelu_inverse(xd, GAIN) - NS * nz.double()[None, None]
        ref.append(dict(g=gref, gz=ref_gz,
                        dot=(rd * xd).sum((0, 2, 3)), dot_abs=(rd * xd).abs().sum((0, 2, 3)),
                        acc=rd.sum((0, 2, 3)), acc_abs=rd.abs().sum((0, 2, 3)),
                        P=torch.stack([ref_R[:, 0] - NS * ref_R[:, 1], ref_R[:, 2]], 1),
                        P_abs=torch.stack([(gzd * zt).abs().sum((0, 2, 3)), gzd.abs().sum((0, 2, 3))], 1)))
    return dict(gz_in=gz_in, d_in=d_in, xin=xin, add=add, w=w, wscale=wscale, s=s, noise=noise, ref=ref)


def test_support_predicate():
    from dge_amd import ops
    for hw in (4, 8, 16, 32):
        assert ops.up_dgrad_small_supported(8, hw, hw, 512, 512, ops.BF16), hw
    assert ops.up_dgrad_small_supported(1, 12, 20, 128, 512, ops.BF16) and ops.up_dgrad_small_supported(2, 8, 8, 64, 256, ops.BF16)
    assert not ops.up_dgrad_small_supported(8, 64, 64, 512, 512, ops.BF16)
    assert not ops.up_dgrad_small_supported(8, 16, 16, 512, 512, ops.F32)
    assert not ops.up_dgrad_small_supported(8, 16, 16, 512, 128, ops.BF16)       # C = 128
    assert not ops.up_dgrad_small_supported(8, 16, 16, 32, 512, ops.BF16)        # N = 32
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        assert not ops.up_dgrad_small_supported(8, 16, 16, 512, 512, ops.BF16)
    finally:
        ops.set_deterministic(was)


def test_packed_copy_unit_by_unit():
    """pack_up_dgrad_small against a torch restatement: unit u = bf16(scale * w[:, :, 2-ky, 2-kx])^T, (ky, kx) = the walk order, stored
    as 32 x 16 (n, k) fragment blocks of 1 KiB, lane (n % 32) + 32 ((k % 16) / 8) holding 8 consecutive k"""
    from dge_amd import ops
    g = torch.Generator(device=DEV).manual_seed(5)
    for C, N in ((256, 64), (512, 128)):
        w = torch.randn(C, N, 3, 3, device=DEV, generator=g)
        got = ops.pack_up_dgrad_small(w, ops.BF16, 0.7)
        assert tuple(got.shape) == (9, N, C) and got.dtype == torch.bfloat16 and got._dge_frag
        flat = got.reshape(9, N // 32, C // 16, 2, 32, 8)                   # [unit][n / 32][k / 16][(k % 16) / 8][n % 32][k % 8]
        for u, (ky, kx) in enumerate(ops.UP_DGRAD_SMALL_UNITS):
            want = (w[:, :, 2 - ky, 2 - kx] * 0.7).to(torch.bfloat16).t().contiguous()          # [n][k]
            want = want.reshape(N // 32, 32, C // 16, 2, 8).permute(0, 2, 3, 1, 4)
            assert torch.equal(flat[u], want), u
    assert sorted(ops.UP_DGRAD_SMALL_UNITS) == [(a, b) for a in range(3) for b in range(3)]


def _run(ops, c, B, N, with_prep, new):
    st, P = ops.SlotStats(B, N, DEV), ops.SlotStats(B, N, DEV)
    prep = dict(gain=GAIN, noise=c["noise"], ns=torch.tensor([NS], device=DEV), stats=P) if with_prep else None
    z = ops.fir_t2d(c["gz_in"], c["d_in"])
    if new:
        out = ops.up_dgrad_small(z, ops.pack_up_dgrad_small(c["w"], ops.BF16, c["wscale"]), c["s"], c["add"], st, c["xin"], prep=prep)
    else:
        out = ops.conv2d(z, ops.pack_conv_weight(c["w"], ops.PACK_UPT2D_DGRAD, ops.BF16, c["wscale"]), N, 3, in_t2d=True, out_scale=c["s"],
                         addend=c["add"], add_scale=1.0, stats=st, dot_src=c["xin"], prep=prep)
    return out, st.buf.sum(0).cpu().double(), (P.buf.sum(0).cpu().double() if with_prep else None)


@pytest.mark.nondet
@pytest.mark.parametrize("with_prep", [False, True])
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("C,N,B,H,W,psn", SHAPES, ids=IDS)
def test_up_dgrad_small_vs_oracle(C, N, B, H, W, psn, with_add, with_prep):
    """Every sample and every pixel.  Bounds: the ones test_fullsize_gpu.py holds the phase-form launches of these layers to.  With
    prep (test_data_gradient_with_fused_tail_backward_fullsize): values within one bf16 rounding with slack 6e-3 of the maximum (Z =
    FIR^T(g_z) * d is rounded to bf16 once before the MFMAs), dot statistics and prep sums 7.9e-3 of the sum of |terms| (its reason: a
    4^2 layer has 16 terms per sum, no averaging).  Without prep (UP_DGRADS, phase-form rows): 7.5e-3 of the maximum, and both
    statistics 8e-4 of the sum of |terms| where a sum has the >= 1024 pixels of that test's smallest row (32^2) to average the operand
    roundings over - the grids below it keep the 7.9e-3 of the few-term sums."""
    from dge_amd import ops
    from dge_amd._lib import last_kernel
    c = _case(C, N, B, H, W, psn, with_add)
    out, stc, Pt = _run(ops, c, B, N, with_prep, new=True)
    assert last_kernel() == f"conv_small<bf16,8,8,64,{C}>+t2d" + ("+prep" if with_prep else "")
    assert tuple(out.shape) == (B, H, W, N)
    dot_bound = 7.9e-3 if (with_prep or H * W < 1024) else 8e-4
    for b in range(B):
        r = c["ref"][b]
        got = _nchw(out, b)
        want = (r["gz"] if with_prep else r["g"]).float()
        viol = _one_rounding(got, want, slack=6e-3)
        e_dot = ((stc[b, :, 0] - r["dot"]).abs() / r["dot_abs"]).max().item()
        print(f"MEAS up_dgrad_small {(C, N, B, H, W)} add={with_add} prep={with_prep} b={b} rounding_viol={viol:.3e} "
              f"relmax={_relmax(got, want):.3e} dot={e_dot:.3e}", end="")
        assert viol <= 0, (b, viol)
        assert e_dot < dot_bound, (b, e_dot)
        if with_prep:
            e_p = ((Pt[b] - r["P"]).abs() / r["P_abs"]).max().item()
            print(f" prep={e_p:.3e}")
            assert e_p < 7.9e-3, (b, e_p)
        else:
            e_acc = ((stc[b, :, 1] - r["acc"]).abs() / r["acc_abs"]).max().item()
            print(f" acc={e_acc:.3e}")
            assert _relmax(got, want) < 7.5e-3, b
            assert e_acc < dot_bound, (b, e_acc)


# Operands and rounding points are those of the launch it replaces, only the f32 summation order differs (4 K quarters x 9 units
# against conv_igemm's chunk order).  Measured on an MI355X over all 24 cases (the MEAS lines): outputs at most 3.36e-3 of the maximum -
# an output moves by one bf16 step where the f32 sum sits on a rounding boundary - so twice that is capped at one bf16 step, 2^-8;
# dot statistics at most 6.8e-7 and prep sums 6.2e-7 of the largest sum: bound at twice the larger, 1.4e-6
OLD_ROUTE_OUT, OLD_ROUTE_STATS = 2.0 ** -8, 1.4e-6


@pytest.mark.nondet
@pytest.mark.parametrize("with_prep", [False, True])
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("C,N,B,H,W,psn", SHAPES, ids=IDS)
def test_up_dgrad_small_vs_the_route_it_replaces(C, N, B, H, W, psn, with_add, with_prep):
    from dge_amd import ops
    c = _case(C, N, B, H, W, psn, with_add)
    a, sa, pa = _run(ops, c, B, N, with_prep, new=True)
    b, sb, pb = _run(ops, c, B, N, with_prep, new=False)
    e_out = ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()
    cols = slice(0, 1) if with_prep else slice(0, 2)                      # (with prep the second column is not written)
    e_st = ((sa[..., cols] - sb[..., cols]).abs().max() / sb[..., cols].abs().max()).item()
    e_p = ((pa - pb).abs().max() / pb.abs().max()).item() if with_prep else 0.0
    print(f"MEAS up_dgrad_small vs conv2d+t2d {(C, N, B, H, W)} add={with_add} prep={with_prep} out={e_out:.3e} stats={e_st:.3e} prep_sums={e_p:.3e}")
    assert e_out <= OLD_ROUTE_OUT, e_out
    assert e_st < OLD_ROUTE_STATS and e_p < OLD_ROUTE_STATS, (e_st, e_p)


@pytest.mark.parametrize("side", [False, True], ids=["main", "side-stream"])
def test_hooks_record_the_launch(side):
    """ops.PROFILE / ops.KERNEL_LOG (tests/test_ops_hooks_gpu.py): a hooked launch computes the same bits and leaves one entry each,
    on the main stream and on a side stream"""
    from dge_amd import ops
    C, N, B, H, W = 256, 64, 2, 8, 8
    c = _case(C, N, B, H, W, False, True)
    wp = ops.pack_up_dgrad_small(c["w"], ops.BF16, c["wscale"])
    z = ops.fir_t2d(c["gz_in"], c["d_in"])
    run = lambda: ops.up_dgrad_small(z, wp, c["s"], c["add"], ops.SlotStats(B, N, DEV), c["xin"])
    y0 = run()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
    prof, log = [], []
    with torch.cuda.stream(stream):
        ops.PROFILE, ops.KERNEL_LOG = prof, log
        try:
            y1 = run()
        finally:
            ops.PROFILE, ops.KERNEL_LOG = None, None
        handle = ops._stream().value
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)
    assert len(prof) == 1 and len(prof[0]) == 5
    e0, e1, fl, tag, nb = prof[0]
    assert fl == 2.0 * 9 * C * N * H * W * B and tag == (B, H, W, 4 * C, N, 3, False, True)
    assert nb == sum(t.numel() * t.element_size() for t in (z, y1, c["add"], c["xin"], wp))
    assert [(n, s.value) for n, s in log] == [(f"conv_small<bf16,8,8,64,{C}>+t2d", handle)]
    assert e0.elapsed_time(e1) >= 0


def test_launch_is_capturable_in_a_graph():
    from dge_amd import ops
    C, N, B, H, W = 256, 64, 2, 8, 8
    c = _case(C, N, B, H, W, False, True)
    wp = ops.pack_up_dgrad_small(c["w"], ops.BF16, c["wscale"])
    z = ops.fir_t2d(c["gz_in"], c["d_in"])
    st = torch.zeros(B, N, 2, device=DEV)
    y0 = ops.up_dgrad_small(z, wp, c["s"], c["add"], st, c["xin"])
    st0 = st.clone()
    st.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y1 = ops.up_dgrad_small(z, wp, c["s"], c["add"], st, c["xin"])
    st.zero_()
    y1.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)
    assert ((st - st0).abs().max() / st0.abs().max()).item() < 1e-5


@pytest.mark.nondet
def test_synthesis_backward_takes_the_new_route_for_its_low_up_layers(monkeypatch):
    """A 32^2 generator whose layers are all 512 -> 512 (fmaps_base 16384): its up layers 1, 3, 5 run on input grids 4^2, 8^2, 16^2.
    g_wp of the synthesis backward in the default (atomics) mode with the switch on and off against the autograd gradient of
    oracle/ref_torch.py's synthesis (tests/golden holds none for this generator), bound of
    test_s2_gpu.py::test_synthesis_grad_wp_vs_reference_golden (bf16: 8e-2).  Switch on: the new kernel for exactly those three layers
    and no space-to-depth conv2d call; switch off: today's launches - three space-to-depth conv2d calls, the other conv2d calls unchanged."""
    import dge_amd
    from dge_amd import ops, s2_conv
    assert not ops.is_deterministic()
    kw = dict(fmaps_base=16384, fmaps_max=512)
    Pm = R.fill_s2(s2_shapes(32, **kw), seed=13)
    G = dge_amd.StyleGAN2Generator(32, compute_dtype="bf16", **kw).cuda()
    G.load_state_dict(Pm)
    B = 2
    for i in (1, 3, 5):
        L = getattr(G.synthesis, f"layer{i}")
        assert L.up and (L.in_c, L.out_c) == (512, 512) and ops.up_dgrad_small_supported(B, L.res // 2, L.res // 2, 512, 512, ops.BF16)
    wp0 = R.randn("s2.wp", (B, 8, 512), 5)
    wpr = wp0.clone().requires_grad_(True)
    img_ref = O.s2_synthesis({k: v.float() for k, v in Pm.items()}, wpr)
    gimg = R.randn("s2.gimg", tuple(img_ref.shape), 5, 1.0 / img_ref.numel() ** 0.5)
    (img_ref * gimg).sum().backward()
    want = wpr.grad.float()
    real_conv, real_up = ops.conv2d, ops.up_dgrad_small
    calls, errs = {}, {}
    for on in (True, False):
        monkeypatch.setattr(s2_conv, "UP_DG_SMALL", on)
        seen = dict(conv=[], up=[])
        calls[on] = seen

        def spy_conv(*a, _s=seen, **k):
            out = real_conv(*a, **k)
            _s["conv"].append((bool(k.get("in_s2d")), bool(k.get("in_t2d")), dge_amd._lib.last_kernel()))
            return out

        def spy_up(z, *a, _s=seen, **k):
            out = real_up(z, *a, **k)
            _s["up"].append((z.shape[1] - 1, dge_amd._lib.last_kernel()))
            return out

        monkeypatch.setattr(ops, "conv2d", spy_conv)
        monkeypatch.setattr(ops, "up_dgrad_small", spy_up)
        wp = wp0.cuda().requires_grad_(True)
        img = G.synthesis(wp)["image"]
        seen["conv"].clear()                                               # (the backward's launches only)
        (img * gimg.cuda()).sum().backward()
        errs[on] = ((wp.grad.float().cpu() - want).abs().max() / want.abs().max()).item()
    print(f"MEAS grad_wp up_dgrad_small on {errs[True]:.3e} off {errs[False]:.3e}")
    assert errs[True] < 8e-2 and errs[False] < 8e-2, errs
    name = "conv_small<bf16,8,8,64,512>+t2d+prep"
    assert calls[True]["up"] == [(16, name), (8, name), (4, name)], calls[True]["up"]
    assert not any(s2d or t2d for s2d, t2d, _ in calls[True]["conv"]), calls[True]["conv"]
    assert calls[False]["up"] == []
    assert sum(s2d for s2d, _, _ in calls[False]["conv"]) == 3 and not any(t2d for _, t2d, _ in calls[False]["conv"]), calls[False]["conv"]
    assert [c for c in calls[False]["conv"] if not c[0]] == calls[True]["conv"]
