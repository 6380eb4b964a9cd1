"""dge_affine_bwd_fromrgb_img on its own: the last launch of the E_BIG backward when the input image carries a gradient (backward
of the conditional batch norm in front of block 0's conv_1 - a per-(b,c) affine -, FromRGB data gradient and, with `img`, the
FromRGB parameter reductions in one launch).

Every case is compared with a float64 restatement of the kernel's formulas on the same (dtype-rounded) operands,

    g = a[b,c]*gy + extra_scale*extra[q(p)];  gp = g*lrelu'(x0);  gimg[b,k,p] = sum_c w[c][k]*gp[c]
    out4[c][0..2] = sum_{b,p} gp*img[b,k,p],  out4[c][3] = sum_{b,p} gp

and with the composition it replaces: ops.in_bwd with coefficients (a, 0, 0) -> ops.fromrgb_dgrad -> ops.fromrgb_bwd.  Bound: the
launch's largest error against float64 is at most 2x the composition's on the same operands plus 1e-6 of the largest reference
element (the two sum in different orders and either can be the luckier one at f32; in bf16 the composition also rounds the
gradient w.r.t. x0 between its launches).  Both errors are logged."""
import pytest
import torch

from tests.conftest import meas
from tests.golden import recipe as R

pytestmark = pytest.mark.gpu

B = 2
# (H, W, C): a partly filled workgroup | 8 / 16 chunks per pixel | the small model's last stage (several workgroups per sample) |
# 128 chunks per pixel in f32: a pixel spans two waves (the LDS step of the reduction)
SHAPES = [(6, 10, 16), (8, 8, 64), (64, 64, 32), (4, 6, 512)]
EXTRAS = ["none", "full", "pooled"]


def _case(hwc, cd, extra_kind):
    H, W, C = hwc
    shape = (B, H, W, C)
    tag = f"abi.{H}.{W}.{C}"
    dt = torch.bfloat16 if cd == "bf16" else torch.float32
    dev = "cuda"
    d = dict(gy=R.randn(tag + ".gy", shape, 1).to(dt).to(dev), x0=R.randn(tag + ".x0", shape, 2, 1.0, 0.2).to(dt).to(dev),
             a=R.randn(tag + ".a", (B, C), 7, 0.3, 1.0).to(dev), w=R.randn(tag + ".w", (C, 3, 1, 1), 9).to(dev),
             img=R.randn(tag + ".img", (B, 3, H, W), 10, 0.5).to(dev))
    d["extra"], d["pool"], d["scale"] = None, False, 1.0
    if extra_kind == "full":
        d["extra"], d["scale"] = R.randn(tag + ".ex", shape, 11).to(dt).to(dev), 0.889
    elif extra_kind == "pooled":
        d["extra"], d["pool"], d["scale"] = R.randn(tag + ".exp", (B, H // 2, W // 2, C), 11).to(dt).to(dev), True, 0.25
    return d


def _f64(d):
    f = lambda t: t.double()
    x0 = f(d["x0"])
    C = x0.shape[3]
    g = f(d["a"])[:, None, None, :] * f(d["gy"])
    if d["extra"] is not None:
        ex = f(d["extra"])
        if d["pool"]:
            ex = ex.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        g = g + d["scale"] * ex
    gp = g * torch.where(x0 > 0, 1.0, 0.2)
    gimg = torch.einsum("bhwc,ck->bkhw", gp, f(d["w"]).reshape(C, 3))
    out4 = torch.cat((torch.einsum("bhwc,bkhw->kc", gp, f(d["img"])), gp.sum(dim=(0, 1, 2))[None]), 0)
    return gimg, out4


def _fused(ops, d, with_out4):
    return ops.affine_bwd_fromrgb_img(d["gy"], d["x0"], d["a"], d["w"], d["img"] if with_out4 else None, extra=d["extra"],
                                      extra_pool=d["pool"], extra_scale=d["scale"])


def _composed(ops, d, with_out4):
    from dge_amd.autograd_encbig import _affine_coef
    gx0 = ops.in_bwd(d["gy"], d["x0"], _affine_coef(d["a"]), extra=d["extra"], extra_pool=d["pool"], extra_scale=d["scale"])
    gimg = ops.fromrgb_dgrad(gx0, d["x0"], d["w"])
    return gimg, (ops.fromrgb_bwd(gx0, d["x0"], d["img"], planar=True) if with_out4 else None)


def _err(a, ref):
    return (a.double() - ref).abs().max().item()


@pytest.mark.parametrize("with_out4", [False, True], ids=["data", "fr"])
@pytest.mark.parametrize("extra_kind", EXTRAS)
@pytest.mark.parametrize("cd", ["bf16", "f32"])
@pytest.mark.parametrize("hwc", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_affine_bwd_fromrgb_img_vs_float64_and_composition(hwc, cd, extra_kind, with_out4):
    from dge_amd import ops
    assert ops.affine_bwd_fromrgb_img_supported(hwc[2], ops.BF16 if cd == "bf16" else ops.F32)
    d = _case(hwc, cd, extra_kind)
    ref_img, ref4 = _f64(d)
    gimg, out4 = _fused(ops, d, with_out4)
    cimg, c4 = _composed(ops, d, with_out4)
    torch.cuda.synchronize()
    assert gimg.shape == (B, 3, hwc[0], hwc[1]) and gimg.dtype == torch.float32 and torch.isfinite(gimg).all()
    assert (out4 is not None) == with_out4
    e_k, e_c, top = _err(gimg, ref_img), _err(cimg, ref_img), ref_img.abs().max().item()
    vals = dict(gimg_kernel=e_k, gimg_composed=e_c, gimg_max=top)
    ok = e_k <= 2.0 * e_c + 1e-6 * top
    if with_out4:
        assert out4.shape == (4, hwc[2])
        e4_k, e4_c, top4 = _err(out4, ref4), _err(c4, ref4), ref4.abs().max().item()
        vals.update(out4_kernel=e4_k, out4_composed=e4_c, out4_max=top4)
        ok = ok and e4_k <= 2.0 * e4_c + 1e-6 * top4
    meas(f"affine_bwd_fromrgb_img.{'x'.join(map(str, hwc))}.{cd}.{extra_kind}.{'fr' if with_out4 else 'data'}", **vals)
    assert ok, vals


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "det"])
@pytest.mark.parametrize("hwc,cd", [((6, 10, 16), "bf16"), ((4, 6, 512), "f32"), ((64, 64, 32), "bf16")],
                         ids=["6x10x16-bf16", "4x6x512-f32", "64x64x32-bf16"])
def test_affine_bwd_fromrgb_img_is_the_same_bits_run_to_run(hwc, cd, det):
    """g_img has a fixed summation order in both modes (with and without the parameter reductions); the FromRGB reductions end in
    f32 atomics in the default mode and are the same bits run to run in deterministic mode."""
    from dge_amd import ops
    d = _case(hwc, cd, "pooled")
    was = ops.is_deterministic()
    ops.set_deterministic(det)
    try:
        a_img, a4 = _fused(ops, d, True)
        b_img, b4 = _fused(ops, d, True)
        c_img, _ = _fused(ops, d, False)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    assert torch.equal(a_img, b_img) and torch.equal(a_img, c_img)
    if det:
        assert torch.equal(a4, b4)


def test_affine_bwd_fromrgb_img_refuses_what_it_does_not_cover():
    """A channel count whose 16-byte chunks do not tile a workgroup, or above 512, is an error of the launch, and the predicate says
    so first (the E_BIG backward then takes the composed passes)."""
    from dge_amd import ops
    assert not ops.affine_bwd_fromrgb_img_supported(1024, ops.BF16) and not ops.affine_bwd_fromrgb_img_supported(24, ops.BF16)
    assert ops.affine_bwd_fromrgb_img_supported(64, ops.BF16) and ops.affine_bwd_fromrgb_img_supported(512, ops.F32)
    d = _case((4, 4, 24), "bf16", "none")
    with pytest.raises(ops.DgeError, match="unsupported channel count"):
        _fused(ops, d, False)
