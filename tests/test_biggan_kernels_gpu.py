"""The BigGAN-deep support kernels (csrc/biggan_kernels.hip and the two max-pool kernels of csrc/lpips_kernels.hip), one operation at
a time, against float64 restatements in plain torch on the same operands (bf16 operands: the bf16-rounded values).

Bounds.  Copies and selections are bit-exact.  A bf16 output is computed in f32 and rounded once: |err| <= 2^-8 |ref| on top of the f32
term.  An f32 reduction over n terms gets n * 2^-23 * sum |terms|, per output, from the restatement's own terms.  Results that pass
through __expf / tanhf / sqrtf / a division by a norm have no bound fixed in advance: the same formula is evaluated by plain torch in
f32 on the CPU, its distance to the float64 restatement is the yardstick, and the kernel gets 8 x that (fast intrinsics, another
summation order) plus 2^-22 of the tensor's maximum.  Every test prints the measured error beside its bound (MEAS lines, pytest -rP).

Measured on MI355X, f32, the largest error over the cases (torch's f32 error and the bound of that case in brackets):
  softmax_rows 1.2e-7 (1.2e-7, 1.2e-6), row sums within 1.2e-7 of 1; attention 3.1e-6 at M = 4000 (1.9e-6, 1.6e-5), closest small case
  2.0e-7 of 4.0e-7; self-attention block 1.9e-6 (2.5e-6, 2.1e-5), in bf16 2.5e-2 (2.5e-2, 4.9e-2); cbn_affine a 6.2e-7 (6.2e-7, 7.6e-6),
  b 1.3e-6 (1.3e-6, 1.3e-5); rgb_tanh 6.7e-8 (3.0e-8, 4.8e-7); sn_group sigma 1.1e-6 (1.1e-7, 3.1e-6), u 8.4e-8 (8.4e-8, 8.2e-7),
  v 8.9e-8 (1.1e-6, 8.8e-6), W_eff 2.8e-8 (7.9e-9, 9.2e-8).
Derived bounds, the element closest to its bound (error of bound): softmax_rows_bwd 1.9e-14 of 2.8e-12; slice_up_bwd 7.5e-9 of 3.4e-8;
  rgb_tanh_bwd 1.8e-9 of 2.2e-8; affine_relu_bwd statistics 1.4e-9 of 6.0e-8 (gx: exact in f32); cbn_sn_wgrad_group 2.2e-8 of 1.4e-6.
  The bf16 outputs come as close as one rounding allows (attention 4.83e-4 of 5.02e-4: a value just above a power of two)."""
import types

import pytest
import torch

from tests.conftest import meas
from tests.golden import recipe as R

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -23          # one f32 rounding, relative (the convention of the issue: twice the round-to-nearest half ulp)
UB = 2.0 ** -8            # one bf16 rounding (test_pn_act_bwd_gpu.py)
_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
CDS = ["f32", "bf16"]


def _ep(cd):
    """elements of one 16-byte chunk"""
    return 4 if cd == "f32" else 8


def _check(name, out, ref, fterm, cd, **tags):
    """|out - ref| <= fterm (+ one bf16 rounding of ref for a bf16 output), elementwise; fterm: a number or a tensor like ref."""
    err = (out.double() - ref).abs()
    bound = fterm + (UB * ref.abs() if cd == "bf16" else 0.0)
    bound = bound if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
    over = err - bound
    i = int(over.argmax())
    meas(name, cd=cd, err=err.flatten()[i].item(), bound=bound.flatten()[i].item(), max_err=err.max().item(), **tags)
    assert bool((over <= 0).all()), (name, cd, tags, err.flatten()[i].item(), bound.flatten()[i].item())


def _check_measured(name, out, ref, f32eval, cd, **tags):
    """The bound of a result that passes through a fast intrinsic: 8 x the error of torch's own f32 evaluation + 2^-22 of max |ref|."""
    yard = (f32eval.double() - ref).abs().max().item()
    fterm = 8.0 * yard + 2.0 ** -22 * ref.abs().max().item()
    _check(name, out, ref, fterm, cd, torch_f32=yard, **tags)
    return fterm


class _mode:
    """ops.set_deterministic(on) for a block; the previous mode comes back afterwards"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from dge_amd import ops
        self.was = ops.is_deterministic()
        ops.set_deterministic(self.on)

    def __exit__(self, *exc):
        from dge_amd import ops
        ops.set_deterministic(self.was)


# ------------------------------------------------------------------ 1. softmax_rows_ / softmax_rows_bwd_
def _scores(cd, Rn, M):
    """about +-8; with more than one row, row 0 holds one entry at +60 and the rest near -60"""
    s = R.randn(f"bk.sm.{Rn}.{M}", (Rn, M), 31, 3.0)
    if Rn > 1:
        s[0] = -60.0 + 0.5 * R.randn(f"bk.sm.spike.{M}", (M,), 32)
        s[0, M // 2] = 60.0
    return s.to(_DT[cd])


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("Rn", [1, 5, 9])
def test_softmax_rows_and_its_backward(cd, Rn):
    """M = 1, 63, 64, 65, 200: one key, an idle lane, one full trip, a tail of one key, three trips and a ragged fourth; R % 4 != 0 leaves
    empty waves in the last workgroup.  Backward on the kernel's own P.
    Measured (f32): forward 1.2e-7 at most (the spike row, torch's f32 softmax the same) against 1.2e-6; row sums within 1.2e-7 of 1."""
    from dge_amd import ops
    for M in (1, 63, 64, 65, 200):
        s = _scores(cd, Rn, M)
        ref = torch.softmax(s.double(), dim=-1)
        p = ops.softmax_rows_(s.clone().cuda())
        assert p.dtype == s.dtype and p.shape == s.shape
        pc = p.cpu()
        fterm = _check_measured("softmax_rows", pc, ref, torch.softmax(s.float(), dim=-1), cd, R=Rn, M=M)
        if cd == "f32":
            rs = (pc.double().sum(dim=-1) - 1.0).abs().max().item()
            meas("softmax_rows_sum", R=Rn, M=M, err=rs, bound=fterm)
            assert rs <= fterm, (M, rs, fterm)
        if Rn > 1:
            assert pc[0].double().argmax().item() == M // 2 and abs(pc[0, M // 2].item() - 1.0) <= UB        # the spike row
        gp = R.randn(f"bk.sm.g.{Rn}.{M}", (Rn, M), 33).to(_DT[cd])
        P, G = pc.double(), gp.double()
        dot_abs = (P * G).abs().sum(dim=-1, keepdim=True)
        gref = P * (G - (P * G).sum(dim=-1, keepdim=True))
        gs = ops.softmax_rows_bwd_(p, gp.clone().cuda())
        _check("softmax_rows_bwd", gs.cpu(), gref, (M + 1) * U32 * P * (G.abs() + dot_abs), cd, R=Rn, M=M)


# ------------------------------------------------------------------ 2. attention
def _qkv(cd, B, N, M, D, DV):
    dt = _DT[cd]
    q = R.randn(f"bk.at.q.{B}.{N}.{D}", (B, N, D), 34, 3.0 / D ** 0.5).to(dt)        # unscaled scores of about +-8
    k = R.randn(f"bk.at.k.{B}.{M}.{D}", (B, M, D), 35).to(dt)
    v = R.randn(f"bk.at.v.{B}.{M}.{DV}", (B, M, DV), 36).to(dt)
    return q, k, v


def _attention_case(cd, B, N, M, D, DV):
    from dge_amd import ops
    q, k, v = _qkv(cd, B, N, M, D, DV)
    ref = torch.softmax(q.double() @ k.double().transpose(1, 2), dim=-1) @ v.double()
    f32 = torch.softmax(q.float() @ k.float().transpose(1, 2), dim=-1) @ v.float()
    o = ops.attention(q.cuda(), k.cuda(), v.cuda())
    assert o.dtype == q.dtype and tuple(o.shape) == (B, N, DV)
    _check_measured("attention", o.cpu(), ref, f32, cd, BN=B * N, M=M, D=D, DV=DV)


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("B,N", [(1, 1), (3, 5)])
def test_attention_kernel_key_tails_and_channel_tails(cd, B, N):
    """M = 1, 63, 65, 200 (a dropped tail key at M = 65 moves every output by about 1/65 of its size), D = 1, 16, 70 (one trip and a
    ragged second trip of the query load), DV = 1, 64, 100 (idle lanes, one trip, a ragged second trip); 3 x 5 queries leave one
    wave of the last workgroup empty and read the keys of three samples.
    Measured (f32): closest case 2.0e-7 against 4.0e-7 (M = 200, D = 16, DV = 1; torch's f32 evaluation 4.6e-8)."""
    for M in (1, 63, 65, 200):
        for D in (1, 16, 70):
            for DV in (1, 64, 100):
                _attention_case(cd, B, N, M, D, DV)


@pytest.mark.parametrize("cd", CDS)
def test_attention_kernel_at_the_largest_admitted_size(cd):
    """M = 4000, D = 96: 4 waves x (96 + 4000) floats = exactly 64 KiB of LDS.  Measured (f32): 3.1e-6 against 1.6e-5 (torch 1.9e-6)."""
    _attention_case(cd, 2, 2, 4000, 96, 64)


def test_attention_kernel_refuses_what_does_not_fit_the_lds():
    from dge_amd import ops
    q = torch.zeros((1, 4, 16), dtype=torch.float32, device="cuda")
    k = torch.zeros((1, 4096, 16), dtype=torch.float32, device="cuda")
    with pytest.raises(ops.DgeError, match="attention"):
        ops.attention(q, k, torch.zeros((1, 4096, 8), dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()


_GAMMA = 4.0


def _attn_block():
    """A hand-filled SelfAttn of 128 channels on the GPU and its four W_eff = W / sigma_max(W) in f32.  The W_eff are parked on the
    _SN holders the way sn_prepare() parks them, so the block and the restatement read the same weights to the bit."""
    from dge_amd.biggan_generator import SelfAttn
    A = SelfAttn(128, eps=1e-4)
    A.gamma.data.fill_(_GAMMA)
    A = A.cuda().eval()
    ws = []
    for name in ("theta", "phi", "g", "o_conv"):
        sn = getattr(A, "snconv1x1_" + name)
        w = R.randn(f"bk.sa.{name}", tuple(sn.weight_orig.shape), 61, 0.05)
        weff = (w.double() / torch.linalg.matrix_norm(w.view(w.shape[0], -1).double(), ord=2)).float()
        sn.__dict__["_prep"] = (weff.cuda(), None, None, None)
        ws.append(weff.view(w.shape[0], -1))
    return A, ws


def _pool_nhwc(t):
    B, H, W, Cc = t.shape
    return t.reshape(B, H // 2, 2, W // 2, 2, Cc).amax(dim=(2, 4))


def _block_eval(x, ws, gamma, rnd, fdt, route):
    """out = x + gamma * conv_o(softmax(theta phi^T) g) (reference biggan_generator.py SelfAttn :75-97) in `fdt` arithmetic; `rnd` is applied
    wherever the route stores a tensor (the kernel route keeps scores and probabilities in registers / LDS)."""
    B, H, W, Cc = x.shape
    wth, wph, wg, wo = [w.to(fdt) for w in ws]
    xf = x.to(fdt)
    theta = rnd(xf @ wth.t()).reshape(B, H * W, -1)
    phi = _pool_nhwc(rnd(xf @ wph.t())).reshape(B, H * W // 4, -1)
    g = _pool_nhwc(rnd(xf @ wg.t())).reshape(B, H * W // 4, -1)
    s = theta @ phi.transpose(1, 2)
    p = torch.softmax(rnd(s), dim=-1) if route == "conv" else torch.softmax(s, dim=-1)
    o = rnd((rnd(p) if route == "conv" else p) @ g).reshape(B, H, W, -1)
    return rnd(xf + gamma * (o @ wo.t()))


@pytest.mark.parametrize("route", ["kernel", "conv"])
@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("size", ["16x16", "small"])
def test_self_attention_block_on_both_routes(size, cd, route, monkeypatch):
    """SelfAttn.run in eval mode, once on attention_kernel (DGE_ATTN_KERNEL=1) and once on the production route
    (conv2d -> softmax_rows_ -> conv2d), against a float64 restatement of the block on the same operands (x and the four W / sigma in
    the compute dtype).  128 channels: D = 16, DV = 64; 16 x 16 gives M = 64.  The second shape is the smallest one conv2d takes with
    M < 64: the score and P V launches need Cout = M and Cin = M to be multiples of 8 (f32: 4 x 8, M = 8) or 16 (bf16: 8 x 8, M = 16).
    Yardstick: the same chain in plain torch on the CPU, in f32 (f32: 8 x its error + 2^-22 of the maximum) or in f32 with a bf16 rounding
    wherever the route stores a tensor (bf16: the kernels make the same roundings in number and kind and differ by the accumulation
    order, which moves single roundings by one ulp: 2 x its maximum error)."""
    from dge_amd import ops
    if route == "kernel":
        monkeypatch.setenv("DGE_ATTN_KERNEL", "1")
    else:
        monkeypatch.delenv("DGE_ATTN_KERNEL", raising=False)
    H, W = (16, 16) if size == "16x16" else ((4, 8) if cd == "f32" else (8, 8))
    dt = _DT[cd]
    A, ws = _attn_block()
    ws = [w.to(dt) for w in ws]
    x = R.randn(f"bk.sa.x.{H}.{W}", (2, H, W, 128), 63).to(dt)
    ident = lambda t: t
    ref = _block_eval(x, ws, _GAMMA, ident, torch.float64, route)
    emul = _block_eval(x, ws, _GAMMA, ident if cd == "f32" else (lambda t: t.to(dt).float()), torch.float32, route)
    with torch.no_grad():
        out = A.run(x.cuda(), ops.F32 if cd == "f32" else ops.BF16, False)
    assert out.dtype == dt and out.shape == x.shape
    err = (out.cpu().double() - ref).abs().max().item()
    yard = (emul.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    # what the attention adds to x must be visible above the bound, or the comparison says nothing about it
    attn = (ref - x.double()).abs().max().item()
    bound = 8.0 * yard + 2.0 ** -22 * scale if cd == "f32" else 2.0 * yard
    meas("self_attention_block", cd=cd, route=route, H=H, W=W, err=err, torch_same_format=yard, bound=bound, attn_term=attn)
    assert attn > 4 * bound, (attn, bound)
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------ 3. maxpool2 / maxpool2_bwd
def _pool_operands(cd, H, W, Cc):
    """x: a post-ReLU tensor on an integer grid (exact in bf16): equal maxima inside windows and whole windows of zeros"""
    x = torch.relu(torch.round(R.randn(f"bk.mp.x.{H}.{W}.{Cc}", (2, H, W, Cc), 37, 1.2)))
    x[0, 0:2, 0:2, 0] = 0.0                                        # a window of zeros: the gradient belongs to its first element
    x[1, 0, 0, 1], x[1, 0, 1, 1], x[1, 1, 0, 1], x[1, 1, 1, 1] = 1.0, 2.0, 2.0, 0.0      # a tie whose first arg-max is not element 0
    gy = R.randn(f"bk.mp.g.{H}.{W}.{Cc}", (2, H // 2, W // 2, Cc), 38)
    add = R.randn(f"bk.mp.a.{H}.{W}.{Cc}", (2, H, W, Cc), 39)
    return x.to(_DT[cd]), gy.to(_DT[cd]), add.to(_DT[cd])


def _windows(x):
    """[B,OH,OW,C,4] with the window's elements in row-major order"""
    B, H, W, Cc = x.shape
    OH, OW = H // 2, W // 2
    return x[:, :2 * OH, :2 * OW].reshape(B, OH, 2, OW, 2, Cc).permute(0, 1, 3, 5, 2, 4).reshape(B, OH, OW, Cc, 4)


def _pool_bwd_ref(gy, x, add, relu):
    """the gradient lands on the first arg-max of the window in row-major order; rows / columns outside every window get the addend
    alone; then the ReLU mask [x > 0] on the complete gradient"""
    B, H, W, Cc = x.shape
    OH, OW = H // 2, W // 2
    w = _windows(x)
    eq = w == w.amax(dim=-1, keepdim=True)
    first = eq & (eq.cumsum(dim=-1) == 1)
    route = (first.double() * gy[..., None]).reshape(B, OH, OW, Cc, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * OH, 2 * OW, Cc)
    gx = torch.zeros_like(x)
    gx[:, :2 * OH, :2 * OW] = route
    if add is not None:
        gx = gx + add
    return gx * (x > 0) if relu else gx


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("HW", [(2, 2), (4, 6), (5, 7)])
def test_maxpool2_and_where_its_gradient_lands(cd, HW):
    """Forward bit-exact; backward without an addend and every f32 backward bit-exact (one exact selection, one f32 addition); bf16 with an
    addend within one bf16 rounding of the exact sum.  The float64 routing is also what torch's max_pool2d autograd does."""
    from dge_amd import ops
    H, W = HW
    for Cc in (_ep(cd), 24, 64):
        x, gy, add = _pool_operands(cd, H, W, Cc)
        w = _windows(x.double())
        eq = w == w.amax(dim=-1, keepdim=True)
        assert bool((eq.sum(dim=-1) > 1).any()) and bool((w == 0).all(dim=-1).any()) and bool((eq[..., 1:] & ~eq[..., :1]).any())
        y = ops.maxpool2(x.cuda())
        assert torch.equal(y.cpu(), w.amax(dim=-1).to(x.dtype)), Cc
        xa = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        torch.nn.functional.max_pool2d(xa, 2).backward(gy.double().permute(0, 3, 1, 2))
        assert torch.equal(xa.grad.permute(0, 2, 3, 1), _pool_bwd_ref(gy.double(), x.double(), None, False))
        for relu in (False, True):
            for a in (None, add):
                ref = _pool_bwd_ref(gy.double(), x.double(), None if a is None else a.double(), relu)
                gx = ops.maxpool2_bwd(gy.cuda(), x.cuda(), addend=None if a is None else a.cuda(), relu=relu).cpu()
                if cd == "f32" or a is None:
                    assert torch.equal(gx, ref.to(x.dtype)), (Cc, relu, a is None)
                else:
                    _check("maxpool2_bwd", gx, ref, 0.0, cd, H=H, W=W, C=Cc, relu=float(relu))


# ------------------------------------------------------------------ 4. slice_up / slice_up_bwd
@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("up", [0, 1])
@pytest.mark.parametrize("HW", [(1, 1), (3, 5)])
def test_slice_up_and_its_adjoint(cd, up, HW):
    """Forward: a copy.  Backward: gx (non-zero before) + the 2^up x 2^up block sum in channels < Cout (5 terms at the most: within
    5 * 2^-23 * sum |terms|, plus one bf16 rounding), channels >= Cout bit-identical."""
    from dge_amd import ops
    H, W = HW
    f = 1 << up
    Cin = 16
    for Cout in (8, 16):
        x = R.randn(f"bk.su.x.{H}.{W}", (2, H, W, Cin), 43).to(_DT[cd])
        y = ops.slice_up(x.cuda(), Cout, up)
        ref = x[..., :Cout].repeat_interleave(f, dim=1).repeat_interleave(f, dim=2)
        assert torch.equal(y.cpu(), ref), (Cout, up)
        gy = R.randn(f"bk.su.g.{H}.{W}.{Cout}.{up}", (2, H * f, W * f, Cout), 44).to(_DT[cd])
        gx0 = R.randn(f"bk.su.gx.{H}.{W}", (2, H, W, Cin), 45).to(_DT[cd])
        gx = ops.slice_up_bwd(gy.cuda(), gx0.clone().cuda(), up).cpu()
        assert torch.equal(gx[..., Cout:], gx0[..., Cout:]), (Cout, up)
        blk = gy.double().reshape(2, H, f, W, f, Cout)
        gref = gx0[..., :Cout].double() + blk.sum(dim=(2, 4))
        terms = gx0[..., :Cout].double().abs() + blk.abs().sum(dim=(2, 4))
        _check("slice_up_bwd", gx[..., :Cout], gref, (f * f + 1) * U32 * terms, cd, H=H, W=W, Cout=Cout, up=up)


# ------------------------------------------------------------------ 5. cbn_affine
def _cbn_ref(scale, offset, mean, var, eps, fdt):
    a = (1.0 + scale.to(fdt)) / torch.sqrt(var.to(fdt) + eps)
    return a, offset.to(fdt) - mean.to(fdt) * a


@pytest.mark.parametrize("layout", ["contiguous", "shared", "slices"])
def test_cbn_affine_layouts(layout):
    """a = (1 + scale) / sqrt(var + eps), b = offset - mean * a for [B,C] rows, [1,C] rows and column slices of one wide matrix (row
    stride != C).  Measured (C = 300, slices): a 6.2e-7 against 7.6e-6 (torch's f32 evaluation 6.2e-7), b 1.3e-6 against 1.3e-5 (1.3e-6)."""
    from dge_amd import ops
    Cs, B, eps = (1, 7, 300), 3, 1e-4
    wide = R.randn("bk.cbn.wide", (B, 2 * sum(Cs) + 4), 46).cuda()
    col = 1
    for Cc in Cs:
        if layout == "slices":
            scale, offset = wide[:, col:col + Cc], wide[:, col + Cc + 1:col + 2 * Cc + 1]
            col += 2 * Cc + 1
            assert scale.stride(0) != Cc
        else:
            Bq = B if layout == "contiguous" else 1
            scale, offset = R.randn(f"bk.cbn.s.{Cc}", (Bq, Cc), 47).cuda(), R.randn(f"bk.cbn.o.{Cc}", (Bq, Cc), 48).cuda()
        mean = R.randn(f"bk.cbn.m.{Cc}", (Cc,), 49).cuda()
        var = (R.randn(f"bk.cbn.v.{Cc}", (Cc,), 50).abs() + 0.05).cuda()
        a, b = ops.cbn_affine(scale, offset, mean, var, eps)
        assert a.shape == scale.shape and b.shape == scale.shape
        ra, rb = _cbn_ref(scale.cpu(), offset.cpu(), mean.cpu(), var.cpu(), eps, torch.float64)
        fa, fb = _cbn_ref(scale.cpu(), offset.cpu(), mean.cpu(), var.cpu(), eps, torch.float32)
        _check_measured("cbn_affine_a", a.cpu(), ra, fa, "f32", layout=layout, C=Cc)
        _check_measured("cbn_affine_b", b.cpu(), rb, fb, "f32", layout=layout, C=Cc)


def test_cbn_affine_refuses_a_strided_inner_axis():
    from dge_amd import ops
    wide = torch.ones((3, 16), dtype=torch.float32, device="cuda")
    one = torch.ones((8,), dtype=torch.float32, device="cuda")
    with pytest.raises(ops.DgeError, match="cbn_affine"):
        ops.cbn_affine(wide[:, ::2], wide[:, 1::2], one, one, 1e-4)
    with pytest.raises(ops.DgeError, match="cbn_affine"):
        ops.cbn_affine(wide[:, :8], torch.ones((3, 8), dtype=torch.float32, device="cuda"), one, one, 1e-4)      # two row strides


# ------------------------------------------------------------------ 6. rgb_tanh / rgb_tanh_bwd
@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("HW", [(3, 5), (17, 19)])
def test_rgb_tanh_and_its_backward(cd, HW):
    """C = 3 (the launcher asks for C >= 3 only, for either dtype: scalar loads), 8, 16; 2 x 15 pixels leave most of one workgroup idle,
    2 x 323 pixels end in a ragged third one.  The backward is 3 f32 roundings (t*t, 1 - t^2, the product) of |g| (1 + t^2) and writes
    exact zeros to channels >= 3.  Measured: forward 6.7e-8 against 4.8e-7 (torch's f32 tanh 3.0e-8)."""
    from dge_amd import ops
    H, W = HW
    for Cc in (3, 8, 16):
        x = R.randn(f"bk.rgb.x.{H}.{W}.{Cc}", (2, H, W, Cc), 51, 1.5).to(_DT[cd])
        img = ops.rgb_tanh(x.cuda())
        assert img.dtype == torch.float32 and tuple(img.shape) == (2, 3, H, W)
        x3 = x[..., :3].permute(0, 3, 1, 2)
        _check_measured("rgb_tanh", img.cpu(), torch.tanh(x3.double()), torch.tanh(x3.float()), "f32", H=H, W=W, C=Cc, src=cd)
        gimg = R.randn(f"bk.rgb.g.{H}.{W}", (2, 3, H, W), 52)
        gy = ops.rgb_tanh_bwd(gimg.cuda(), img, Cc, ops.F32 if cd == "f32" else ops.BF16).cpu()
        assert gy.dtype == _DT[cd] and tuple(gy.shape) == (2, H, W, Cc)
        t = img.cpu().double()
        ref = (gimg.double() * (1.0 - t * t)).permute(0, 2, 3, 1)
        _check("rgb_tanh_bwd", gy[..., :3], ref, 3 * U32 * (gimg.double().abs() * (1.0 + t * t)).permute(0, 2, 3, 1), cd, H=H, W=W, C=Cc)
        assert bool((gy[..., 3:] == 0).all()), Cc


# ------------------------------------------------------------------ 7. affine_relu_bwd
def _affine_operands(cd, B, H, W, Cc, dev="cpu"):
    """|a| >= 0.5; a*x + b at least 0.2 away from 0 except where it is built to be exactly 0 (x = 0 in a channel with b = 0)."""
    dt = _DT[cd]
    tag = f"{B}.{H}.{W}.{Cc}"
    ra = R.randn(f"bk.ar.a.{tag}", (B, Cc), 53).to(dev)
    a = torch.where(ra > 0, 1.0, -1.0) * (0.5 + R.randn(f"bk.ar.a2.{tag}", (B, Cc), 54).to(dev).abs())
    b = 0.5 * R.randn(f"bk.ar.b.{tag}", (B, Cc), 55).to(dev)
    b[:, 1::4] = 0.0
    x = R.randn(f"bk.ar.x.{tag}", (B, H, W, Cc), 56).to(dt).to(dev)
    gu = R.randn(f"bk.ar.g.{tag}", (B, H, W, Cc), 57).to(dt).to(dev)
    a4, b4 = a.double()[:, None, None, :], b.double()[:, None, None, :]
    near = (a4 * x.double() + b4).abs() < 0.25
    x = torch.where(near, x.float() + torch.sign(a)[:, None, None, :], x.float()).to(dt)          # moves a*x + b up by |a| >= 0.5
    zero = R.randn(f"bk.ar.z.{tag}", (B, H, W, Cc), 58).to(dev) > 1.15
    zero[0, 0, 0, 1] = True
    zero[..., 0::4] = False; zero[..., 2::4] = False; zero[..., 3::4] = False
    x = torch.where(zero, torch.zeros((), dtype=dt, device=dev), x)
    pre = a4 * x.double() + b4
    assert int(zero.sum()) > 0 and bool((pre[zero] == 0).all()) and pre[~zero].abs().min().item() >= 1e-3
    assert bool((gu[zero] != 0).all())
    return gu, x, a, b, pre


def _affine_check(cd, gu, x, a, b, pre, gx, st, **tags):
    B, H, W, Cc = x.shape
    m = (pre > 0).double()                                         # strict: the entries at exactly 0 are masked out
    a4 = a.double()[:, None, None, :]
    _check("affine_relu_bwd_gx", gx, m * a4 * gu.double(), U32 * (m * a4 * gu.double()).abs(), cd, **tags)
    t0, t1 = (m * gu.double() * x.double()).reshape(B, H * W, Cc), (m * gu.double()).reshape(B, H * W, Cc)
    ref = torch.stack([t0.sum(dim=1), t1.sum(dim=1)], dim=-1)
    bound = H * W * U32 * torch.stack([t0.abs().sum(dim=1), t1.abs().sum(dim=1)], dim=-1)
    assert tuple(st.shape) == (B, Cc, 2)
    _check("affine_relu_bwd_stats", st, ref, bound, "f32", src=cd, **tags)


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("HW", [(1, 1), (3, 3), (5, 7)])
def test_affine_relu_bwd_in_both_reduction_modes(cd, HW):
    """C = one chunk (256 pixel slots per workgroup), 64, and 2048 (one pixel per workgroup trip; in f32 two channel groups of 1024:
    blockIdx.z = 1 - a missing second group leaves gx and the statistics of channels >= 1024 unwritten or zero).  Two runs in
    deterministic mode agree bit for bit; both modes meet the same bound."""
    from dge_amd import ops
    H, W = HW
    for Cc in (_ep(cd), 64, 2048):
        gu, x, a, b, pre = _affine_operands(cd, 2, H, W, Cc)
        dev = [t.cuda() for t in (gu, x, a, b)]
        runs = []
        for det in (True, True, False):
            with _mode(det):
                gx, st = ops.affine_relu_bwd(*dev)
            runs.append((gx.cpu(), st.cpu()))
            _affine_check(cd, gu, x, a, b, pre, gx.cpu(), st.cpu(), H=H, W=W, C=Cc, det=float(det))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), Cc


def test_affine_relu_bwd_refuses_what_overflows_the_deterministic_workspace():
    """B = 96, HW = 96, C = 2048 in bf16: 96 domains x 96 slots x 4096 floats = 37.7 M floats, more than the 32 Mi floats of the
    deterministic-mode workspace.  Before the launcher asked dge_det_fits, det_slot() trapped on the device here.  In the default mode the
    same shape runs and meets the bound of the small cases."""
    from dge_amd import ops
    gu, x, a, b, pre = _affine_operands("bf16", 96, 8, 12, 2048, dev="cuda")
    with _mode(True):
        with pytest.raises(ops.DgeError, match="affine_relu_bwd"):
            ops.affine_relu_bwd(gu, x, a, b)
        torch.cuda.synchronize()
    with _mode(False):
        gx, st = ops.affine_relu_bwd(gu, x, a, b)
    _affine_check("bf16", gu, x, a, b, pre, gx, st, H=8, W=12, C=2048, B=96)


# ------------------------------------------------------------------ 8. dge_cbn_sn_wgrad_group
def _cbn_norms(B, K):
    """Three stand-in conditional batch norms (C = 5, 130, 300) with their ctx dicts and per-(b,c) sums.  Mostly positive operands: the
    sum <gw, W> over C*K terms then is of the size of its sum of magnitudes, and the n * 2^-23 * sum |terms| bound stays below what a
    lost row share, a lost tail of k or a lost second trip over the rows (C > 256) would change."""
    norms = []
    for Cc in (5, 130, 300):
        sns = {}
        for key in ("scale", "offset"):
            w = (R.randn(f"bk.cg.w.{Cc}.{key}", (Cc, K), 64).abs() * 0.05 + 0.01).cuda()
            u = torch.nn.functional.normalize(R.randn(f"bk.cg.u.{Cc}.{key}", (Cc,), 65).abs() + 0.1, dim=0).cuda()
            v = torch.nn.functional.normalize(R.randn(f"bk.cg.v.{Cc}.{key}", (K,), 66).abs() + 0.1, dim=0).cuda()
            sigma = torch.dot(u, w @ v)
            sns[key] = (types.SimpleNamespace(weight_orig=w), dict(u=u, v=v, sigma=sigma))
        bn = types.SimpleNamespace(scale=sns["scale"][0], offset=sns["offset"][0])
        ctx = dict(mean=(0.3 * R.randn(f"bk.cg.m.{Cc}", (Cc,), 67)).cuda(), rstd=(R.randn(f"bk.cg.r.{Cc}", (Cc,), 68).abs() + 0.5).cuda(),
                   sn_sc=sns["scale"][1], sn_of=sns["offset"][1])
        dots = (R.randn(f"bk.cg.d.{B}.{Cc}", (B, Cc, 2), 69).abs() + 0.1).cuda()
        norms.append((bn, ctx, dots, f"norm{Cc}"))
    return norms


def _cbn_grad_ref(bn, ctx, dots, cond, key):
    """gy -> gw = gy^T cond -> (gw - <gw, W> / sigma * u v^T) / sigma in float64, and the f32 bound of it from the same terms"""
    d = dots.double().cpu()
    B, Cc = d.shape[0], d.shape[1]
    c = cond.double().cpu()
    K = c.shape[1]
    mean, rstd = ctx["mean"].double().cpu(), ctx["rstd"].double().cpu()
    sn = ctx["sn_sc" if key == "scale" else "sn_of"]
    wm = getattr(bn, key).weight_orig.double().cpu()
    u, v, sigma = sn["u"].double().cpu(), sn["v"].double().cpu(), sn["sigma"].double().cpu()
    if key == "scale":
        gy, gy_abs = (d[:, :, 0] - d[:, :, 1] * mean) * rstd, (d[:, :, 0].abs() + (d[:, :, 1] * mean).abs()) * rstd
    else:
        gy, gy_abs = d[:, :, 1], d[:, :, 1].abs()
    gw = gy.t() @ c
    e_gw = (B + 3) * U32 * (gy_abs.t() @ c.abs())                  # B terms, each behind the three roundings of gy
    dot = (gw * wm).sum()
    e_dot = Cc * K * U32 * (gw * wm).abs().sum() + (e_gw * wm.abs()).sum()
    uv = torch.outer(u, v)
    ref = (gw - dot / sigma * uv) / sigma
    bound = (e_gw + e_dot / sigma.abs() * uv.abs() + 4 * U32 * (gw.abs() + (dot / sigma * uv).abs())) / sigma.abs()
    return ref, bound, (dot / sigma * uv / sigma).abs().max().item()


@pytest.mark.parametrize("B", [1, 3])
def test_cbn_param_grads_group_against_float64_and_the_per_norm_path(B):
    """K = 100 leaves a ragged second trip of the k loop; C = 300 takes a second trip of the per-entry row sum; six table entries of three
    sizes exercise the row -> entry search."""
    from dge_amd import autograd_encbig as AE
    K = 100
    cond = (R.randn(f"bk.cg.c.{B}", (B, K), 70).abs() + 0.1).cuda()
    norms = _cbn_norms(B, K)
    grads, single = {}, {}
    pend = []
    for bn, ctx, dots, name in norms:
        AE._cbn_param_grads(bn, ctx, dots, cond, grads, name, pend=pend)
        AE._cbn_param_grads(bn, ctx, dots, cond, single, name, pend=None)
    assert len(pend) == 3 and not grads
    AE._cbn_param_grads_flush(pend, cond, grads)
    assert not pend and set(grads) == set(single) and len(grads) == 6
    for bn, ctx, dots, name in norms:
        for key in ("scale", "offset"):
            ref, bound, uv_term = _cbn_grad_ref(bn, ctx, dots, cond, key)
            g = grads[f"{name}.{key}.weight_orig"].cpu()
            assert g.shape == ref.shape
            assert uv_term > 50 * bound.max().item()          # the u v^T term carries weight: a wrong <gw, W> cannot hide below the bound
            _check("cbn_sn_wgrad_group", g, ref, bound, "f32", B=B, C=ref.shape[0], key=key)
            _check("cbn_sn_wgrad_per_norm", single[f"{name}.{key}.weight_orig"].cpu(), ref, bound, "f32", B=B, C=ref.shape[0], key=key)


# ------------------------------------------------------------------ 9. sn_prepare (dge_sn_group)
_SN_SHAPES = [(1, 1), (3, 5), (64, 256), (65, 257), (130, 1000), (300, 7)]


def _sn_fill(sn, tag):
    """weights N(0, 0.05); u / v after two float64 power iterations from a random start, so that sigma = u . W v is O(1) in eval mode too"""
    O, K = sn.weight_orig.shape
    w = R.randn(f"bk.sn.w.{tag}", (O, K), 71, 0.05)
    u = R.randn(f"bk.sn.u.{tag}", (O,), 72).double()
    for _ in range(2):
        v = torch.nn.functional.normalize(w.double().t() @ u, dim=0)
        u = torch.nn.functional.normalize(w.double() @ v, dim=0)
    sn.weight_orig.data.copy_(w); sn.weight_u.copy_(u.float()); sn.weight_v.copy_(v.float())


def _sn_module(shapes, eps=1e-4):
    from dge_amd.biggan_generator import _SN
    m = torch.nn.Module()
    m.sns = torch.nn.ModuleList([_SN(s, False, eps) for s in shapes])
    m.skipme = torch.nn.Module()
    m.skipme.inner = _SN((9, 11), False, eps)
    for i, sn in enumerate(list(m.sns) + [m.skipme.inner]):
        _sn_fill(sn, f"{i}.{tuple(sn.weight_orig.shape)}")
    m.__dict__["_sn_skip"] = ("skipme.",)
    return m.cuda()


def _power_iteration(w, u, v, eps, training, fdt):
    """torch.nn.utils.spectral_norm: train: v = normalize(W^T u), u = normalize(W v); sigma = u . (W v); W_eff = W / sigma"""
    w, u, v = w.to(fdt), u.to(fdt), v.to(fdt)
    if training:
        v = torch.nn.functional.normalize(w.t() @ u, dim=0, eps=eps)
        u = torch.nn.functional.normalize(w @ v, dim=0, eps=eps)
    sigma = torch.dot(u, w @ v)
    return w / sigma, sigma, u, v


def _sn_check(mod, training, tag):
    from dge_amd.biggan_generator import sn_prepare
    sns = list(mod.sns)
    before = [(sn.weight_orig.detach().cpu(), sn.weight_u.cpu().clone(), sn.weight_v.cpu().clone()) for sn in sns]
    skip_u, skip_v = mod.skipme.inner.weight_u.clone(), mod.skipme.inner.weight_v.clone()
    sn_prepare(mod, training)
    torch.cuda.synchronize()
    assert torch.equal(mod.skipme.inner.weight_u, skip_u) and torch.equal(mod.skipme.inner.weight_v, skip_v)
    assert mod.skipme.inner.__dict__.get("_prep") is None
    for sn, (w, u0, v0) in zip(sns, before):
        weff, sigma, us, vs = sn.__dict__["_prep"]
        sn.__dict__["_prep"] = None
        ref = _power_iteration(w, u0, v0, sn.eps, training, torch.float64)
        f32 = _power_iteration(w, u0, v0, sn.eps, training, torch.float32)
        O, K = w.shape
        assert weff.shape == w.shape
        got = (weff.cpu(), sigma.cpu().reshape(()), sn.weight_u.cpu(), sn.weight_v.cpu())
        for what, g, r, f in zip(("w_eff", "sigma", "u", "v"), got, ref, f32):
            _check_measured("sn_group_" + what, g, r, f, "f32", O=O, K=K, train=float(training), mode=tag)
        assert torch.equal(us.cpu(), sn.weight_u.cpu()) and torch.equal(vs.cpu(), sn.weight_v.cpu())      # the snapshots for the backward
        if not training:
            assert torch.equal(sn.weight_u.cpu(), u0) and torch.equal(sn.weight_v.cpu(), v0)


@pytest.mark.parametrize("det", [False, True])
def test_sn_prepare_against_a_float64_power_iteration(det):
    """O = 65, 130, 300 take more than one row slab of sn_wtu (a lost slab moves v by far more than the bound), K = 257 and 1000 more than
    one block of k with a ragged last one; (1, 1) and (3, 5) leave most of every launch idle.  Train mode (one power iteration, buffers
    updated in place), then eval mode on the updated buffers (u / v bit-identical afterwards)."""
    mod = _sn_module(_SN_SHAPES)
    with _mode(det):
        _sn_check(mod, True, "det" if det else "atomics")
        _sn_check(mod, False, "det" if det else "atomics")


@pytest.mark.parametrize("det", [True, False])
def test_sn_prepare_group_larger_than_the_deterministic_workspace(det):
    """One weight of (32768, 256) (BigGAN-deep's gen_z) with 80 of (8, 1024): sized by the group's maxima, sn_wtu takes 4 x 81 = 324
    domains x 512 slots x 256 floats = 42.5 M floats in deterministic mode, more than the workspace of 32 Mi floats.  dge_sn_group used
    to launch that at once and det_slot() trapped on the device; it now walks the table in sub-ranges that fit (64 + 17 entries)."""
    mod = _sn_module([(32768, 256)] + [(8, 1024)] * 80)
    with _mode(det):
        _sn_check(mod, True, "det" if det else "atomics")
