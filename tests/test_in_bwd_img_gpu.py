"""dge_in_bwd_fromrgb_img on its own: the last launch of the encoder backward when the input image carries a gradient
(instance-norm backward of block 0's conv_1, FromRGB data gradient and, with `img`, the FromRGB parameter gradients in one launch).

Every case is compared with a float64 restatement of the kernel's formulas on the same (dtype-rounded) operands,

    g = A*gy + Bc*x0 + Cc + extra_scale*extra[q(p)];  gp = g*lrelu'(x0);  gimg[b,k,p] = sum_c w[c][k]*gp[c]
    out4[c][0..2] = sum_{b,p} gp*img[b,k,p],  out4[c][3] = sum_{b,p} gp

and with the composition it replaces: ops.in_bwd -> ops.fromrgb_dgrad -> ops.fromrgb_bwd.  Bounds (none fixed in advance, both
errors are logged): f32 - the kernel only reorders f32 sums, so it is within 2x the composition's own error against float64;
bf16 - the composition rounds the gradient w.r.t. x0 to bf16 between its launches and the kernel does not, so the kernel's error
is at most the composition's."""
import pytest
import torch

from tests.conftest import meas
from tests.golden import recipe as R

pytestmark = pytest.mark.gpu

# [B,H,W,C], dtype: one workgroup with two chunks per pixel in bf16 | HW no multiple of the pixels per workgroup | 8 / 16 chunks |
# 128 chunks per pixel (the cross-wave reduction) | grid capped, second trip of the two-pixel loop partly out of range
SHAPES = [((2, 8, 8, 16), "bf16"), ((2, 8, 8, 16), "f32"), ((1, 6, 6, 16), "bf16"), ((1, 6, 6, 16), "f32"), ((2, 8, 8, 64), "bf16"),
          ((2, 8, 8, 64), "f32"), ((1, 4, 4, 512), "bf16"), ((1, 4, 4, 512), "f32"), ((2, 256, 384, 16), "bf16"), ((2, 256, 384, 16), "f32")]
EXTRAS = ["none", "unpooled", "pooled"]


def _case(shape, cd, extra_kind):
    """Operands on the device (activations rounded to the compute dtype) and the float64 coefficients of the instance-norm backward
    (the math of in_bwd_coef) from the same sources the launch reads."""
    B, H, W, C = shape
    tag = f"ibi.{B}.{H}.{W}.{C}"
    dt = torch.bfloat16 if cd == "bf16" else torch.float32
    dev = "cuda"
    N = H * W
    d = dict(
        gy=R.randn(tag + ".gy", shape, 1).to(dt).to(dev), x0=R.randn(tag + ".x0", shape, 2, 1.0, 0.2).to(dt).to(dev),
        dots=(R.randn(tag + ".dots", (B, C, 2), 3) * N ** 0.5).to(dev), gms=R.randn(tag + ".gms", (B, 2 * C), 4).to(dev),
        musig=torch.cat((R.randn(tag + ".mu", (B, C), 5, 0.3), R.randn(tag + ".sg", (B, C), 6, 0.1, 1.0).abs() + 0.5), 1).to(dev),
        sc=(R.randn(tag + ".sc", (B, C), 7, 0.1, 1.0).abs() + 0.5).to(dev), sh=R.randn(tag + ".sh", (B, C), 8, 0.3).to(dev),
        w=R.randn(tag + ".w", (C, 3, 1, 1), 9).to(dev), img=R.randn(tag + ".img", (B, 3, H, W), 10, 0.5).to(dev))
    d["extra"], d["pool"], d["scale"] = None, False, 1.0
    if extra_kind == "unpooled":
        d["extra"], d["scale"] = R.randn(tag + ".ex", shape, 11).to(dt).to(dev), 0.889
    elif extra_kind == "pooled":
        d["extra"], d["pool"], d["scale"] = R.randn(tag + ".exp", (B, H // 2, W // 2, C), 11).to(dt).to(dev), True, 0.25
    return d


def _f64(d, shape):
    B, H, W, C = shape
    N = H * W
    f = lambda t: t.double()
    r, s = f(d["sc"]), f(d["sh"])
    S2, S1 = f(d["dots"])[..., 0], f(d["dots"])[..., 1]
    m1, m2 = S1 / N, (r * S2 + s * S1) / N
    mu, sg = f(d["musig"])[:, :C], f(d["musig"])[:, C:]
    gmu, gsg = f(d["gms"])[:, :C], f(d["gms"])[:, C:]
    k = gsg / N / sg
    A, Bc, Cc = r, -r * r * m2 + k, -r * m1 - r * m2 * s + gmu / N - k * mu
    v = lambda t: t[:, None, None, :]
    x0 = f(d["x0"])
    g = v(A) * f(d["gy"]) + v(Bc) * x0 + v(Cc)
    if d["extra"] is not None:
        ex = f(d["extra"])
        if d["pool"]:
            ex = ex.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        g = g + d["scale"] * ex
    gp = g * torch.where(x0 > 0, 1.0, 0.2)
    gimg = torch.einsum("bhwc,ck->bkhw", gp, f(d["w"]).reshape(C, 3))
    out4 = torch.cat((torch.einsum("bhwc,bkhw->kc", gp, f(d["img"])), gp.sum(dim=(0, 1, 2))[None]), 0)
    return gimg, out4


def _l2(a, ref):
    return ((a.double() - ref).norm() / (ref.norm() + 1e-300)).item()


def _coef(d, shape):
    return (d["dots"], d["gms"], d["musig"], d["sc"], d["sh"], shape[1] * shape[2])


def _fused(ops, d, shape, with_out4):
    return ops.in_bwd_fromrgb_img(d["gy"], d["x0"], _coef(d, shape), d["w"], d["img"] if with_out4 else None, extra=d["extra"],
                                  extra_pool=d["pool"], extra_scale=d["scale"])


def _composed(ops, d, shape, with_out4):
    gx0 = ops.in_bwd(d["gy"], d["x0"], _coef(d, shape), extra=d["extra"], extra_pool=d["pool"], extra_scale=d["scale"])
    gimg = ops.fromrgb_dgrad(gx0, d["x0"], d["w"])
    return gimg, (ops.fromrgb_bwd(gx0, d["x0"], d["img"], planar=True) if with_out4 else None)


@pytest.mark.parametrize("with_out4", [False, True], ids=["data", "fr"])
@pytest.mark.parametrize("extra_kind", EXTRAS)
@pytest.mark.parametrize("shape,cd", SHAPES, ids=[f"{'x'.join(map(str, s))}-{c}" for s, c in SHAPES])
def test_in_bwd_fromrgb_img_vs_float64_and_composition(shape, cd, extra_kind, with_out4):
    from dge_amd import ops
    assert ops.in_bwd_fromrgb_img_supported(shape[3], ops.BF16 if cd == "bf16" else ops.F32)
    d = _case(shape, cd, extra_kind)
    ref_img, ref4 = _f64(d, shape)
    gimg, out4 = _fused(ops, d, shape, with_out4)
    cimg, c4 = _composed(ops, d, shape, with_out4)
    torch.cuda.synchronize()
    assert gimg.shape == (shape[0], 3, shape[1], shape[2]) and gimg.dtype == torch.float32
    assert (out4 is not None) == with_out4
    e_k, e_c = _l2(gimg.cpu(), ref_img.cpu()), _l2(cimg.cpu(), ref_img.cpu())
    vals = dict(gimg_kernel=e_k, gimg_composed=e_c)
    factor = 2.0 if cd == "f32" else 1.0
    assert torch.isfinite(gimg).all()
    ok = e_k <= factor * e_c
    if with_out4:
        assert out4.shape == (4, shape[3])
        e4_k, e4_c = _l2(out4.cpu(), ref4.cpu()), _l2(c4.cpu(), ref4.cpu())
        vals.update(out4_kernel=e4_k, out4_composed=e4_c)
        ok = ok and e4_k <= factor * e4_c
    meas(f"in_bwd_fromrgb_img.{'x'.join(map(str, shape))}.{cd}.{extra_kind}.{'fr' if with_out4 else 'data'}", **vals)
    assert ok, vals


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "det"])
@pytest.mark.parametrize("shape,cd", [((2, 8, 8, 16), "bf16"), ((1, 4, 4, 512), "f32"), ((2, 256, 384, 16), "bf16")],
                         ids=["2x8x8x16-bf16", "1x4x4x512-f32", "2x256x384x16-bf16"])
def test_in_bwd_fromrgb_img_is_the_same_bits_run_to_run(shape, cd, det):
    """g_img has a fixed summation order in both modes; the FromRGB reductions end in f32 atomics in the default mode and are the
    same bits run to run in deterministic mode."""
    from dge_amd import ops
    d = _case(shape, cd, "pooled")
    was = ops.is_deterministic()
    ops.set_deterministic(det)
    try:
        a_img, a4 = _fused(ops, d, shape, True)
        b_img, b4 = _fused(ops, d, shape, True)
        c_img, _ = _fused(ops, d, shape, False)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    assert torch.equal(a_img, b_img) and torch.equal(a_img, c_img)
    if det:
        assert torch.equal(a4, b4)


def test_in_bwd_fromrgb_img_refuses_what_it_does_not_cover():
    """A channel count whose 16-byte chunks do not tile a workgroup is an error of the launch, and the predicate says so first."""
    from dge_amd import ops
    assert not ops.in_bwd_fromrgb_img_supported(1024, ops.BF16) and not ops.in_bwd_fromrgb_img_supported(24, ops.BF16)
    d = _case((1, 4, 4, 24), "bf16", "none")
    with pytest.raises(ops.DgeError, match="unsupported channel count"):
        _fused(ops, d, (1, 4, 4, 24), False)
