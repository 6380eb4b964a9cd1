"""StyleGAN2 mapping and truncation, differentiable w.r.t. z (stylegan2_generator.py): against the reference's own w, wp and z
gradients (tests/golden/s2_mapping_grad.npz, tools/gen_golden_s2_mapping.py), in both reduction modes and through both adjoint
kernels (dge_mapping_bwd, dge_mapping_bwd_wide)."""
import pytest
import torch

from tests.conftest import MODES, golden, meas
from tests.golden import recipe as R
from tests.s2z_models import S2Z_KW, s2z_state_dict

pytestmark = pytest.mark.gpu
TRUNC = [("t8", 0.7, 8), ("t10", 0.7, 10), ("none", None, None)]


def relerr(a, b):
    a = a.detach().float().cpu()
    b = torch.as_tensor(b).float()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def generator(wide=False, cd="f32"):
    import dge_amd
    G = dge_amd.StyleGAN2Generator(64, compute_dtype=cd, **S2Z_KW).cuda()
    G.load_state_dict(s2z_state_dict())
    G.eval()
    G.mapping.wide_bwd = wide
    return G


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("wide", [False, True])
def test_generator_z_gradient_vs_reference_golden(wide, mode):
    """G(z) with z.requires_grad in eval mode (it raised DgeError before): the image gradient reaches z through the synthesis'
    wp gradient and the mapping adjoint.  Bound: the f32 bound test_synthesis_grad_wp_vs_reference_golden has for g_wp."""
    g = golden("s2_mapping_grad.npz")
    G = generator(wide)
    z = torch.as_tensor(g["z"]).cuda().requires_grad_(True)
    out = G(z, trunc_psi=0.7, trunc_layers=8, randomize_noise=False)
    img = out["image"]
    assert abs(float(img.detach().norm()) - float(g["image_norm"])) < 2e-4 * float(g["image_norm"])
    with torch.no_grad():
        ref = G(z.detach(), trunc_psi=0.7, trunc_layers=8, randomize_noise=False)
    assert torch.equal(out["w"], ref["w"]) and torch.equal(out["wp"], ref["wp"]) and torch.equal(img, ref["image"])
    gi = R.randn("s2map.gi", tuple(img.shape), 83).cuda()
    (img * gi).sum().backward()
    e = relerr(z.grad, g["dz_image"])
    meas(f"s2_mapping.dz_image.{'wide' if wide else 'one'}.{mode}", rel=e)
    assert e < 1e-3, e


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("tag,psi,layers", TRUNC)
def test_mapping_truncation_dz_vs_reference_golden(tag, psi, layers, wide, mode):
    g = golden("s2_mapping_grad.npz")
    G = generator(wide)
    z = torch.as_tensor(g["z"]).cuda().requires_grad_(True)
    w = G.mapping(z)["w"]
    wp = G.truncation(w, psi, layers)
    assert w.requires_grad and wp.requires_grad
    with torch.no_grad():
        w0 = G.mapping(z.detach())["w"]
        wp0 = G.truncation(w0, psi, layers)
    assert torch.equal(w, w0) and torch.equal(wp, wp0)          # bit-identical to the no-grad path
    assert relerr(w, g["w"]) < 1e-5 and relerr(wp, g["wp_" + tag]) < 1e-5
    gw = R.randn("s2map.gw." + tag, tuple(wp.shape), 82).cuda()
    (wp * gw).sum().backward()
    e = relerr(z.grad, g["dz_" + tag])
    meas(f"s2_mapping.dz_{tag}.{'wide' if wide else 'one'}.{mode}", rel=e)
    assert e <= 1e-5, e
    # w alone (the mapping module on its own) is differentiable too: the `none` case's gradient with one row
    if tag == "none":
        z2 = torch.as_tensor(g["z"]).cuda().requires_grad_(True)
        (G.mapping(z2)["w"] * gw.sum(dim=1)).sum().backward()
        assert relerr(z2.grad, g["dz_none"]) <= 1e-5


def test_train_mode_side_effects_still_refuse_a_z_gradient():
    from dge_amd import ops
    G = generator()
    G.train()
    z = R.randn("s2map.ztrain", (2, 512), 3).cuda().requires_grad_(True)
    with pytest.raises(ops.DgeError, match="w_avg"):
        G(z)
    with pytest.raises(ops.DgeError, match="style mixing"):
        G(z, w_moving_decay=1.0)
    with pytest.raises(ops.DgeError, match="w_avg") as ei:
        G(z, style_mixing_prob=0)
    assert "style mixing" not in str(ei.value)
    # no side effect active: train mode works and changes nothing
    avg = G.truncation.w_avg.clone()
    img = G(z, w_moving_decay=1.0, style_mixing_prob=0)["image"]
    img.sum().backward()
    assert torch.isfinite(z.grad).all() and float(z.grad.abs().max()) > 0 and torch.equal(G.truncation.w_avg, avg)


def test_no_grad_call_logs_the_launches_it_logged():
    """A z without grad: dge_pixelnorm (not logged), eight dge_linear, dge_truncation (not logged), then the synthesis - the dense
    entries of KERNEL_LOG are the same with a z that requires grad (the forward issues the same launches) and hold no adjoint."""
    from dge_amd import ops
    G = generator()
    z = R.randn("s2map.zlog", (2, 512), 3).cuda()

    def logged(zz, grad):
        log = []
        ops.KERNEL_LOG = log
        try:
            with torch.set_grad_enabled(grad):
                G(zz, trunc_psi=0.7, trunc_layers=8)
        finally:
            ops.KERNEL_LOG = None
        return [n for n, _ in log]
    plain = logged(z, True)
    assert plain[:8] == ["dge_linear"] * 8 and not any("mapping_bwd" in n for n in plain)
    assert logged(z, False) == plain
    assert logged(z.clone().requires_grad_(True), True) == plain
