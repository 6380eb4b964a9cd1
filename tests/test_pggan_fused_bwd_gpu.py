"""PGGANGenerator(z, fused_backward=True): the latent gradient with ops.pixelnorm_act_bwd in place of every
[nearest_up2_bwd ->] pixelnorm_nhwc_bwd -> act_bwd group, against the reference's autograd (tests/golden/pggan_grad.npz) within the
bounds tests/test_pggan.py sets for the composed path; and the default call's launch sequence against a restatement of what
`_backward` issued before the keyword existed."""
import pytest
import torch

from tests.conftest import golden, meas
from tests.golden import recipe as R
from tests.test_pggan import _l2rel, small_params

pytestmark = pytest.mark.gpu

_TRACED = ("torgb_bwd", "pixelnorm_nhwc_bwd", "act_bwd", "conv2d", "nearest_up2_bwd", "pixelnorm_act_bwd", "nhwc_to_nchw", "linear_t")


def _generator(cd):
    from dge_amd.pggan_generator import PGGANGenerator
    G = PGGANGenerator(32, fmaps_base=1024, fmaps_max=64, compute_dtype=cd).cuda()
    G.load_state_dict(small_params())
    for p in G.parameters():
        p.requires_grad_(False)
    return G


def _trace(monkeypatch):
    """Every call of the ops the generator backward is made of, as (op, shapes / dtypes / scalars of its arguments), in call order."""
    from dge_amd import ops
    calls = []

    def sig(v):
        if torch.is_tensor(v):
            return (tuple(v.shape), str(v.dtype))
        if isinstance(v, (bool, int, float, str, type(None))):
            return v
        if isinstance(v, (list, tuple)):
            return tuple(sig(x) for x in v)
        return type(v).__name__

    def wrap(name):
        orig = getattr(ops, name)

        def f(*a, **kw):
            calls.append((name, tuple(sig(v) for v in a), tuple(sorted((k, sig(v)) for k, v in kw.items()))))
            return orig(*a, **kw)
        monkeypatch.setattr(ops, name, f)
    for name in _TRACED:
        wrap(name)
    return calls


@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_fused_latent_gradient_vs_reference_golden(cd, monkeypatch):
    """The bounds of test_pggan.test_hip_latent_gradient_vs_reference_golden (f32: loss 2e-4, g_z L2 3e-3; bf16: cosine 0.98,
    L2 0.2).  The fused backward launches no stand-alone act_bwd above the dense tail and no nearest_up2_bwd."""
    g = golden("pggan_grad.npz")
    G = _generator(cd)
    z = R.randn("pg.z", (2, 512), 51).cuda().requires_grad_(True)
    img = G(z, fused_backward=True)["image"]
    loss = (img.float() * R.randn("pg.gimg", tuple(img.shape), 52).cuda()).sum()
    calls = _trace(monkeypatch)
    loss.backward()
    names = [c[0] for c in calls]
    nconv = names.count("conv2d")
    assert nconv == 7 and names.count("pixelnorm_act_bwd") == nconv, names          # behind torgb_bwd + between the 7 convs
    assert names.count("nearest_up2_bwd") == 0 and names.count("act_bwd") == 1, names          # the dense tail's
    assert names.count("pixelnorm_nhwc_bwd") == 2, names          # in front of layer1 (reads the dense output) and on z
    err = _l2rel(z.grad, g["g_z"])
    cos = torch.nn.functional.cosine_similarity(z.grad.float().cpu().flatten(), torch.as_tensor(g["g_z"]).flatten(), dim=0).item()
    meas("pggan_fused_bwd", cd=cd, l2=err, cos=cos)
    if cd == "f32":
        assert abs(float(loss.detach()) - float(g["loss"])) < 2e-4 * abs(float(g["loss"])) and err < 3e-3, err
    else:
        assert cos > 0.98 and err < 0.2, (cos, err)


def test_fused_f32_equals_composed_f32():
    """In f32 nothing is rounded between the composed launches, so the fused form differs by summation order and FMA contraction
    only: 1e-5 relative L2 on g_z after 7 layers."""
    G = _generator("f32")
    gimg = R.randn("pg.gimg", (2, 3, 32, 32), 52).cuda()
    out = []
    for fused in (False, True):
        z = R.randn("pg.z", (2, 512), 51).cuda().requires_grad_(True)
        (G(z, fused_backward=fused)["image"].float() * gimg).sum().backward()
        out.append(z.grad)
    assert _l2rel(out[1], out[0].cpu().numpy()) < 1e-5


def test_refused_channel_count_takes_the_composed_launches(monkeypatch):
    from dge_amd import ops
    G = _generator("f32")
    gimg = R.randn("pg.gimg", (2, 3, 32, 32), 52).cuda()
    z0 = R.randn("pg.z", (2, 512), 51).cuda()
    z = z0.clone().requires_grad_(True)
    (G(z)["image"].float() * gimg).sum().backward()
    monkeypatch.setattr(ops, "pixelnorm_act_bwd_supported", lambda Cc, dt: Cc != 64)

    def guard(orig):
        def f(g, x, **kw):
            assert x.shape[3] != 64, "fused launch used for a refused channel count"
            return orig(g, x, **kw)
        return f
    monkeypatch.setattr(ops, "pixelnorm_act_bwd", guard(ops.pixelnorm_act_bwd))
    z2 = z0.clone().requires_grad_(True)
    (G(z2, fused_backward=True)["image"].float() * gimg).sum().backward()
    assert _l2rel(z2.grad, z.grad.cpu().numpy()) < 1e-5


def _backward_as_before(G, saved, g_image):
    """What PGGANGenerator._backward(saved, g_image) issued before it learnt `fused`: the same ops, in that order."""
    from dge_amd import ops
    dt = ops.dtype_of(saved["x_last"])
    B = g_image.shape[0]
    O_ = saved["out"]
    ones = torch.ones((B, saved["x_last"].shape[3]), dtype=torch.float32, device=g_image.device)
    g_xn, _ = ops.torgb_bwd(g_image.float().contiguous(), saved["xn_last"], O_.weight.detach().reshape(3, -1), ones, O_.wscale)
    g = ops.pixelnorm_nhwc_bwd(g_xn, saved["x_last"])
    for L, x_in, y, up in reversed(saved["convs"]):
        g_pre = ops.act_bwd(g, y, None, pool=False, scale=1.0) if L.act == ops.ACT_LRELU else g
        g_xn = ops.conv2d(g_pre, L.packed(dt, ops.PACK_DGRAD), L.in_c, 3)
        if up:
            g_xn, _ = ops.nearest_up2_bwd(g_xn)
        g = ops.pixelnorm_nhwc_bwd(g_xn, x_in)
    C0 = G.layer0.out_c
    g_h = ops.nhwc_to_nchw(g.view(B, 1, 1, 16 * C0)).view(B, 4, 4, C0)
    g_hpre = ops.act_bwd(g_h, saved["h"].view(B, 4, 4, C0), None, pool=False, scale=1.0).view(B, 16 * C0)
    wd, _ = G._dense0_weight()
    g_zn = torch.empty((B, G.z_space_dim), dtype=torch.float32, device=g_image.device)
    ops.linear_t(g_hpre, wd, g_zn, scale=G.layer0.wscale)
    return ops.pixelnorm_nhwc_bwd(g_zn.view(B, 1, 1, -1), saved["z"].view(B, 1, 1, -1)).view(B, -1)


@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_default_backward_issues_the_launches_it_issued_before(cd, monkeypatch):
    """Without the keyword (what e_align --mtype 3 runs): the traced op sequence, the KERNEL_LOG sequence and the bits of g_z equal
    those of the restatement above; through autograd the default call gives the same bits again."""
    from dge_amd import ops
    G = _generator(cd)
    z = R.randn("pg.z", (2, 512), 51).cuda()
    gimg = R.randn("pg.gimg", (2, 3, 32, 32), 52).cuda()
    with torch.no_grad():
        _, _, saved = G._run(z, save=True)
        calls = _trace(monkeypatch)
        runs = []
        for fn in (lambda: G._backward(saved, gimg), lambda: _backward_as_before(G, saved, gimg)):
            del calls[:]
            ops.KERNEL_LOG = log = []
            try:
                out = fn()
            finally:
                ops.KERNEL_LOG = None
            torch.cuda.synchronize()
            runs.append((list(calls), [n for n, _ in log], out))
    (calls_a, log_a, out_a), (calls_b, log_b, out_b) = runs
    assert len(calls_a) > 25 and calls_a == calls_b
    assert log_a == log_b
    assert "pixelnorm_act_bwd" not in [c[0] for c in calls_a]
    assert torch.equal(out_a, out_b)
    monkeypatch.undo()
    zg = z.clone().requires_grad_(True)
    (G(zg)["image"].float() * gimg).sum().backward()
    assert torch.equal(zg.grad, out_a)
