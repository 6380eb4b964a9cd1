"""Z-space encoder training (dge_amd.e_align_z, reference ablation_utils/1.E_align_z.py): the mapping network's data gradient
(dge_mapping_bwd), the E_Blur_Z encoder and the two-phase loop, against the reference's own numbers (tools/gen_golden.py sections
mapping_grad, encz_grad, step_z)."""
import os
import sys

import numpy as np
import pytest
import torch

from tests.conftest import golden, with_fixture_params, meas, MODES, ROOT
from tests.golden import recipe as R

pytestmark = pytest.mark.gpu


def relerr(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    return ((a - b).abs().max() / b.abs().max()).item()


def _l2rel(a, b):
    a = a.detach().float().cpu().flatten(); b = torch.as_tensor(np.asarray(b)).float().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _composed():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_e_align_z import composed_mapping_bwd
    return composed_mapping_bwd


def _mapgrad_model(with_buffer):
    import dge_amd.stylegan1 as S
    L = 10
    Gm = S.Mapping(num_layers=L).cuda()
    Gm.load_state_dict({k: R.randn("mapgrad.m." + k, tuple(v.shape), 71, 0.05 if k.endswith("weight") else 0.01)
                        for k, v in Gm.state_dict().items()})
    Gm.buffer1 = R.randn("mapgrad.buffer1", (L, 512), 72, 0.5) if with_buffer else None
    layer_idx = torch.arange(L)[None, :, None]
    ones = torch.ones(layer_idx.shape, dtype=torch.float32)
    return Gm, torch.where(layer_idx < L // 2, 0.7 * ones, ones)


@pytest.mark.parametrize("tag", ["", "_nobuf"])
def test_mapping_dz_vs_reference_golden(tag):
    g = golden("mapping_grad.npz")
    Gm, coefs = _mapgrad_model(tag == "")
    z = R.randn("mapgrad.z", (3, 512), 71).cuda().requires_grad_(True)
    w = Gm(z, coefs_m=coefs)
    assert relerr(w, g["w" + tag]) < 1e-5
    gw = R.randn("mapgrad.gw" + tag, tuple(w.shape), 73).cuda()
    (w * gw).sum().backward()
    err = relerr(z.grad, g["dz" + tag])
    meas("mapping_dz" + tag, rel=err)
    assert err <= 1e-5, err


@pytest.mark.parametrize("tag", ["", "_nobuf"])
def test_mapping_dz_matches_composed_ops_and_is_reproducible(tag):
    from dge_amd import ops
    Gm, coefs = _mapgrad_model(tag == "")
    z = R.randn("mapgrad.z", (3, 512), 71).cuda()
    g = R.randn("mapgrad.gw" + tag, (3, 10, 512), 73).cuda()
    c = coefs.reshape(-1).cuda() if tag == "" else None
    acts = Gm.activations(z)
    dz1 = ops.mapping_bwd(z, Gm.chain(), g, coefs=c, acts=acts)
    dz2 = ops.mapping_bwd(z, Gm.chain(), g, coefs=c, acts=acts)
    assert torch.equal(dz1, dz2)
    # without saved activations the launch recomputes the forward (dge_dense_chain's arithmetic, bit-identical): same masks, same bits
    assert torch.equal(dz1, ops.mapping_bwd(z, Gm.chain(), g, coefs=c))
    ref = _composed()(Gm, z, g, c)
    err = relerr(dz1, ref.cpu())
    meas("mapping_dz_vs_composed" + tag, rel=err)
    assert err < 1e-5, err


def test_differentiable_mapping_forward_is_bit_identical_to_per_layer_launches():
    """Mapping.forward with and without autograd against dge_pixelnorm + 8 dge_linear + dge_lerp_layers, and the one-launch chain
    (dge_dense_chain, the arithmetic dge_mapping_bwd recomputes when it is given no saved activations) against the same."""
    from dge_amd import ops
    Gm, coefs = _mapgrad_model(True)
    z = R.randn("mapgrad.z", (5, 512), 75).cuda()
    x = ops.pixelnorm(z)
    for i in range(8):
        fc = getattr(Gm, "block_%d" % (i + 1)).fc
        x = ops.linear(x, fc.weight.detach(), fc.bias.detach(), act=ops.ACT_LRELU)
    ref = ops.lerp_layers(x, Gm.buffer1.cuda().float().contiguous(), coefs.reshape(-1).cuda())
    with torch.no_grad():
        w_ng = Gm(z, coefs_m=coefs)
    w_ad = Gm(z.clone().requires_grad_(True), coefs_m=coefs)
    assert w_ad.requires_grad
    assert torch.equal(w_ng, ref) and torch.equal(w_ad.detach(), ref)
    assert torch.equal(ops.lerp_layers(ops.dense_chain(z, Gm.chain(), pixelnorm=True), Gm.buffer1.cuda().float().contiguous(),
                                       coefs.reshape(-1).cuda()), ref)


def _encz(cd):
    from dge_amd.encoder_variants import BlurBEZ
    g = golden("encz_grad.npz")
    E = BlurBEZ(startf=32, maxf=512, layer_count=5, compute_dtype=cd).cuda()
    sd = R.fill_encoder({k: list(v.shape) for k, v in E.state_dict().items()}, seed=81)
    for k in sd:
        if k.endswith("blur.weight"):
            sd[k] = E.state_dict()[k].clone()
    E.load_state_dict(with_fixture_params(sd, g))
    return E, g


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_e_blur_z_gradients_vs_reference_golden(cd, mode):
    E, g = _encz(cd)
    img = R.randn("ez.img", (2, 3, 64, 64), 81, 0.5).cuda().requires_grad_(True)
    z, w = E(img)
    assert tuple(z.shape) == (2, 512, 1, 1) and int(w) == 0
    zerr = relerr(z, g["z"])
    loss = (z * R.randn("ez.gz", tuple(z.shape), 83).cuda()).sum()
    loss.backward()
    f32 = cd == "f32"
    assert zerr < (2e-4 if f32 else 3e-2), zerr
    tol, tol_img = (1e-3, 1e-3) if f32 else (0.48, 0.43)       # the bounds of test_hip_e_blur_gradients_vs_reference_golden
    worst, checked = (0.0, None), 0
    for k, p in E.named_parameters():
        if "grad:" + k not in g.files:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        nrm = float(g["norm:" + k])
        mine = p.grad.detach().float().cpu()
        assert abs(float(mine.norm()) - nrm) < tol * nrm + 1e-6, (k, float(mine.norm()), nrm)
        mine = mine if mine.numel() <= 16384 else mine.flatten()[:4096]
        e = _l2rel(mine, g["grad:" + k])
        worst = max(worst, (e, k))
        assert e < tol, (k, e)
        checked += 1
    img_e = _l2rel(img.grad, g["g_img"])
    meas("encz_grads", cd=cd, mode=mode, z=zerr, worst_l2=worst[0], key=worst[1], img_l2=img_e)
    assert checked >= 25 and img_e < tol_img, (checked, img_e)
    # out_z reads the top-left 3x3 window: its weight gradient is the window's, row / column 3 of the trunk get none
    assert float(E.out_z.weight.grad.abs().max()) > 0


def _step_models():
    import dge_amd.stylegan1 as S
    from dge_amd.lpips import LPIPS
    from oracle import lpips_ref as LR
    from tests.test_sg1 import sg1_shapes
    L = 5
    Gs = S.Generator(startf=16, maxf=64, layer_count=L, latent_size=512, compute_dtype="f32").cuda()
    shapes = sg1_shapes(16, 64, L)
    sd = R.fill_encoder(shapes, seed=43)
    blur = torch.tensor([[1., 2., 1.], [2., 4., 2.], [1., 2., 1.]]) / 16.0
    for k in sd:
        if k.endswith("blur.weight"):
            sd[k] = blur.view(1, 1, 3, 3).repeat(shapes[k][0], 1, 1, 1)
    sd["const"] = R.randn("sg1step.const", tuple(shapes["const"]), 43)
    Gs.load_state_dict(sd)
    Gm = S.Mapping(num_layers=2 * L).cuda()
    Gm.load_state_dict({k: R.randn("sg1step.m." + k, tuple(v.shape), 44, 0.05 if k.endswith("weight") else 0.01)
                        for k, v in Gm.state_dict().items()})
    Gm.buffer1 = R.randn("sg1step.buffer1", (2 * L, 512), 44, 0.5)
    for p in list(Gs.parameters()) + list(Gm.parameters()):
        p.requires_grad_(False)
    LP = LPIPS(compute_dtype="f32").cuda()
    LP.load_state_dict(LR.seeded_params(0))
    return Gs, Gm, LP


def test_two_phase_z_step_matches_reference_run():
    """Two iterations of 1.E_align_z.py at reduced size (tests/golden/step_z.npz): image loss through Gs AND Gm into E_Blur_Z,
    LREQAdam, latent loss on z, LREQAdam; every generator noise tensor replayed."""
    from dge_amd.e_align_z import EAlignZStep
    g = golden("step_z.npz")
    Gs, Gm, LP = _step_models()
    E, _ = _encz("f32")
    st = EAlignZStep(Gs, Gm, E, LP, lr=0.0015, batch_size=2)
    nshapes = [tuple(int(v) for v in s if v) for s in g["noise_shapes"].tolist()]
    assert len(nshapes) == 20
    for it in range(2):
        z = R.randn(f"zstep.z{it}", (2, 512), 1)
        nz = [R.randn(f"zstep.it{it}.noise{i}", s, 1) for i, s in enumerate(nshapes)]
        r = st.step(it, z=z, gen_noises=(nz[:10], nz[10:]))
        assert relerr(r["w1"], g[f"it{it}_w1"]) < 1e-4
        errs = dict(z_c2=relerr(r["z_c2"], g[f"it{it}_z_c2"]), w2=relerr(r["w2"], g[f"it{it}_w2"]),
                    imgs2=relerr(r["imgs2"], g[f"it{it}_imgs2"]))
        meas("step_z", it=it, **errs)
        assert errs["z_c2"] < 2e-3 and errs["w2"] < 2e-3 and errs["imgs2"] < 3e-3, (it, errs)
        got = [float(r["loss_imgs"]), float(r["loss_c"])]
        for a, b in zip(got, g[f"it{it}_losses"]):
            assert abs(a - b) < 3e-3 * abs(b), (it, got, g[f"it{it}_losses"])
        sd_e = E.state_dict()
        for key in g.files:
            if key.startswith(f"it{it}_after_phase2:"):
                k = key.split(":", 1)[1]
                assert _l2rel(sd_e[k], g[key]) < 1.5e-3, (it, k, _l2rel(sd_e[k], g[key]))
        assert _l2rel(sd_e["out_z.weight"].flatten()[:4096], g[f"it{it}_after_phase2_head:out_z.weight"]) < 1.5e-3
        assert abs(R.checksum({k: v.cpu() for k, v in sd_e.items()}) - float(g[f"it{it}_param_checksum"])) < 1e-5 * float(g[f"it{it}_param_checksum"])


def test_fullsize_bf16_z_step_runs_and_trains():
    """One bf16 step at StyleGAN1 FFHQ-1024 (startf 16, 9 blocks, batch 2): finite losses, out_z and block 0 move."""
    from dge_amd.e_align_z import EAlignZStep, build_models_z
    Gs, Gm, E, LP = build_models_z(1024, 16, "bf16")
    st = EAlignZStep(Gs, Gm, E, LP, batch_size=2)
    before = {k: E.state_dict()[k].clone() for k in ("out_z.weight", "decode_block.0.conv_1.weight", "FromRGB.from_rgb.weight")}
    r = st.step(0)
    assert tuple(r["imgs2"].shape) == (2, 3, 1024, 1024) and tuple(r["z_c2"].shape) == (2, 512)
    assert np.isfinite(float(r["loss_imgs"])) and np.isfinite(float(r["loss_c"]))
    for k, v in before.items():
        assert not torch.equal(E.state_dict()[k], v), k
