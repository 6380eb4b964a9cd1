"""BigGAN-deep real-image inversion (dge_amd.embedding_v2_biggan.BigEmbedStep) against two iterations of the reference's own
modules (embedding_v2_BigGAN.py:78-165 at reduced size: tests/golden/embed_v2_big.npz, tools/gen_golden_embed_big.py) in mode E,
mode W and mode W with the attention terms, and the refusals of what the loop does not offer."""
import numpy as np
import pytest
import torch

from tests.conftest import MODES, golden, meas
from tests.golden import recipe as R
from oracle import lpips_ref as LR

pytestmark = pytest.mark.gpu
CASES = {"E": ("E", False), "W": ("W", False), "W-att": ("W", True)}
PNAMES = ("decode_block.0.conv_1.weight", "decode_block.2.conv_2.weight", "decode_block.1.conv_3.weight",
          "decode_block.1.batch_norm_1.scale.weight_orig", "decode_block.0.batch_norm_3.offset.weight_orig",
          "decode_block.1.batch_norm_2.scale.weight_u", "decode_block.1.bias_1", "FromRGB.from_rgb.weight", "new_final_2.bias")


def relerr(a, b):
    a = a.detach().float().cpu()
    b = torch.as_tensor(np.asarray(b)).float()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def l2rel(a, b):
    a = a.detach().float().cpu().flatten(); b = torch.as_tensor(np.asarray(b)).float().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def make_models(att, cd="f32"):
    from dge_amd.biggan_generator import BigGAN, BigGANConfig
    from dge_amd.encoder_variants import BigBE
    from dge_amd.lpips import LPIPS
    from tests.test_biggan import SMALL
    G = BigGAN(BigGANConfig.from_dict(SMALL), compute_dtype=cd).cuda()
    G.load_state_dict(R.fill_biggan({n: list(v.shape) for n, v in G.state_dict().items()}, 71))
    E = BigBE(startf=32, maxf=512, layer_count=5, biggan=True, compute_dtype=cd).cuda()
    E.load_state_dict(R.fill_encbig({n: list(v.shape) for n, v in E.state_dict().items()}, 81))
    LP = LPIPS(compute_dtype=cd).cuda()
    LP.load_state_dict(LR.seeded_params(0))
    vgg = None
    if att:
        from dge_amd import grad_cam
        from oracle import gradcam_ref as GR
        cfg = R.GRADCAM_CFG
        ref = GR.VGG16Ref(cfg["widths"], cfg["fc"], cfg["classes"])
        vgg = grad_cam.VGG16(cfg["widths"], cfg["fc"], cfg["classes"], compute_dtype=cd)
        vgg.load_state_dict(GR.seeded_state({k: list(v.shape) for k, v in ref.state_dict().items()}, cfg["seed"]))
        vgg = vgg.cuda()
    return G, E, LP, vgg


def case_noises(g, tag, it):
    """(E(imgs1), E(imgs2)) noise lists of iteration `it` of a golden case."""
    shapes = [tuple(s) for s in g[f"{tag}_noise_shapes"].tolist()]
    s0, s1 = [int(v) for v in g[f"{tag}_noise_split"].tolist()]
    nz = [R.randn(f"embed_v2_big.{tag}.it{it}.noise{i}", s, 2).cuda() for i, s in enumerate(shapes)]
    return (nz[:s0] or None, nz[s0:s1])


def make_step(tag, g, **kw):
    from dge_amd.embedding_v2_biggan import BigEmbedStep
    opt, att = CASES[tag]
    G, E, LP, vgg = make_models(att)
    st = BigEmbedStep(G, E, LP, mode=opt, vgg16=vgg, attention=att, label=30, lr=0.0003, iterations=2, **kw)
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    if opt == "W":
        shapes = [tuple(s) for s in g[f"{tag}_init_noise_shapes"].tolist()]
        st.begin_image(imgs1, noises=[R.randn(f"embed_v2_big.{tag}.init.noise{i}", s, 2).cuda() for i, s in enumerate(shapes)])
    else:
        st.begin_image(imgs1)
    return st, imgs1


# Bounds: those of tests/test_embed_v2_gpu.py::test_embed_v2_loop_matches_reference_run, except where a comment gives the measured
# deterministic f32 value (bound at most 3x it).  `lt`: relative bound of the loss values, 1e-3 in deterministic mode, 3e-3 in the
# default mode, 3x that in iteration 1.
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag", list(CASES))
def test_big_embed_loop_matches_reference_run(tag, mode):
    g = golden("embed_v2_big.npz")
    opt, att = CASES[tag]
    st, imgs1 = make_step(tag, g)
    E = st.E
    assert _train_mode(st) and relerr(st.cond_vector, g[f"{tag}_cond_vector"]) < 1e-5
    if opt == "W":
        assert relerr(st.w1, g[f"{tag}_w0"]) < 1e-3 and relerr(st._const1, g[f"{tag}_const1"]) < 1e-3
        assert all(not p.requires_grad for p in E.parameters())
    lt = 1e-3 if mode == "det" else 3e-3
    for it in range(2):
        calls = []
        orig = st.opt.step

        def spy(*a, **kw):
            calls.append(E.FromRGB.from_rgb.weight.grad.detach().clone() if opt == "E" else st.w1.grad.detach().clone())
            return orig(*a, **kw)
        st.opt.step = spy
        try:
            r = st.step(imgs1, noises=case_noises(g, tag, it))
        finally:
            st.opt.step = orig
        pre = f"{tag}_it{it}"
        gkey = "FromRGB.from_rgb.weight" if opt == "E" else "w1"
        info = r["info_imgs"].cpu().numpy()
        ref_l = g[f"{pre}_losses"]          # loss_msiv, loss_imgs, loss_w, loss_c2, loss_mslv
        got_l = [float(r["loss_msiv"]), float(r["loss_imgs"]), float(r["loss_w"]), float(r["loss_c2"]), float(r["loss_mslv"])]
        e = dict(w1=relerr(r["w1"], g[f"{pre}_w1"]), w1_l2=l2rel(r["w1"], g[f"{pre}_w1"]), w2=relerr(r["w2"], g[f"{pre}_w2"]),
                 imgs2=relerr(r["imgs2"][:, :, ::2, ::2], g[f"{pre}_imgs2"]),
                 imgs2_norm=abs(float(r["imgs2"].norm()) - float(g[f"{pre}_imgs2_norm"])) / float(g[f"{pre}_imgs2_norm"]),
                 const2=relerr(r["const2"], g[f"{pre}_const2"]),
                 const1=relerr(r["const1"], g[f"{pre}_const1"] if opt == "E" else g[f"{tag}_const1"]),
                 losses=max(abs(a - b) / abs(b) for a, b in zip(got_l, ref_l)),
                 grad1=l2rel(calls[0], g[f"{pre}_grad1:{gkey}"]), grad2=l2rel(calls[1], g[f"{pre}_grad2:{gkey}"]))
        if opt == "E":
            ck = R.checksum({k: v.cpu() for k, v in E.state_dict().items() if v.dtype.is_floating_point})
        else:
            ck = R.checksum({"w1": st.w1.detach().cpu()})
        e["checksum"] = abs(ck - float(g[f"{pre}_param_checksum"])) / float(g[f"{pre}_param_checksum"])
        ref_info = g[f"{pre}_info"]          # rows imgs [, mask, Gcam], w, c2; columns mse, mean, std, kl, cos, ssim, lpips
        e["info_imgs"] = max(abs(info[1 + c] - ref_info[0, c]) / (abs(ref_info[0, c]) + 1e-6) for c in (0, 4, 5, 6))
        if att:
            e["mask_2"] = float(np.abs(r["mask_2"].cpu().numpy() - g[f"{pre}_mask_2"]).max())
            ref_a = g[f"{pre}_att_losses"]
            e["att_losses"] = max(abs(float(r["loss_mask"]) - ref_a[0]) / abs(ref_a[0]), abs(float(r["loss_Gcam"]) - ref_a[1]) / abs(ref_a[1]))
        meas(f"embed_v2_big.{tag}.{mode}.it{it}", **e)
        if opt == "W":
            assert e["w1_l2"] < 1e-3 and e["w1"] < 4e-3, (it, e)
        else:
            assert e["w1"] < 1e-3, (it, e)
        assert e["w2"] < (2e-3 if it == 0 else 1e-2), (it, e)
        assert e["imgs2"] < IMGS2_BOUND[opt][it] and e["imgs2_norm"] < 2e-3, (it, e)
        assert e["const2"] < (2e-3 if it == 0 else 1e-2) and e["const1"] < 1e-3, (it, e)
        assert e["losses"] <= (lt if it == 0 else 3 * lt), (it, got_l, ref_l.tolist())
        assert e["info_imgs"] < 1e-2, (it, e)
        # phase 2 and iteration 1 follow sign-like first Adam steps (see test_embed_gpu.py)
        assert e["grad1"] < (5e-3 if it == 0 else 6e-2) and e["grad2"] < 6e-2, (it, e)
        assert e["checksum"] < 2e-4, (it, e)
        if att:      # the bounds of test_gradcam.test_mis_align_iteration_matches_reference_run
            assert e["mask_2"] < 5e-3 and e["att_losses"] < 5e-3, (it, e)
        if opt == "E":
            sd = E.state_dict()
            for k in PNAMES:
                ref = torch.as_tensor(g[f"{pre}_after_phase2:{k}"])
                mine = sd[k].cpu()
                assert abs(float(mine.norm()) - float(g[f"{pre}_after_phase2_norm:{k}"])) < 1e-3 * float(g[f"{pre}_after_phase2_norm:{k}"]), (it, k)
                mine = mine if mine.numel() <= 4096 else mine.flatten()[:4096]
                # beta1 = 0: a step is lr * sign(g)-like; single elements whose gradient is within rounding of zero may step the
                # other way, 2 * lr per phase (see test_step_gpu.test_two_phase_step_biggan_matches_reference_run)
                assert float((mine - ref.reshape(mine.shape)).abs().max()) < 4.2 * 0.0003 * (it + 1), (it, k)
    tr = st.tracker()
    assert tr["iteration"] == 2 and tr["dropped"] == 0


def _train_mode(st):
    """both networks in train mode, the generator frozen"""
    return st.G.training and st.E.training and all(not p.requires_grad for p in st.G.parameters())


# imgs2 (largest error relative to max |imgs2|), iterations 0 / 1.  Mode E, iteration 1: measured 1.75e-2 in deterministic f32
# (2.1e-2 in the default mode) for a w1 that differs by 2.8e-4 - the encoder has taken two sign-like LREQAdam steps (beta1 = 0), and
# its randomly initialised head puts w1 at |w1| ~ 15, far outside BigGAN's truncated-normal range, where the generator amplifies the
# difference (see test_step_gpu.test_two_phase_step_biggan_matches_reference_run, which allows 0.15 there).  Bound: 3x the measured
# deterministic value.  The image's norm stays within 2e-3 (measured 5e-5).
IMGS2_BOUND = {"E": (2e-3, 5.2e-2), "W": (2e-3, 2e-3)}


# ------------------------------------------------------------------ tracker
def test_tracker_arms_at_half_and_follows_the_host_rule():
    """tracker_rules("sg1", iterations): armed at iterations // 2 (min := that loss), a save whenever min > loss * 1.05."""
    from tests.test_embed_v2_gpu import host_track
    g = golden("embed_v2_big.npz")
    st, imgs1 = make_step("W", g, arm_iter=2)
    noises = case_noises(g, "W", 0)
    seq, ws = [], {}
    for i in range(6):
        r = st.step(imgs1, noises)
        seq.append((i, float(r["loss_msiv"]), float(r["w_norm"])))
        ws[i] = r["w1"].clone()
    want, mins = host_track(st.rules, seq, st.rules["init"])
    tr = st.tracker()
    assert [(ev[0], ev[1]) for ev in tr["events"]] == want and tr["iteration"] == 6
    assert tr["min_loss"] == mins[0]
    if want:
        assert torch.equal(tr["best_loss"], ws[want[-1][0]])
    st.begin_image(imgs1)          # a new group: counter, log and minima restart
    tr = st.tracker()
    assert tr["iteration"] == 0 and tr["events"] == [] and tr["min_loss"] == 0.0


# ------------------------------------------------------------------ refusals
def test_capture_independent_and_process_groups_are_refused(monkeypatch):
    from dge_amd import embedding_v2_biggan as M
    g = golden("embed_v2_big.npz")
    st, imgs1 = make_step("W", g)
    with pytest.raises(ValueError, match="hipGraph capture / replay is not offered"):
        st.capture(imgs1)
    with pytest.raises(ValueError, match="hipGraph capture / replay is not offered"):
        st.replay()
    G, E, LP, _ = make_models(False)
    with pytest.raises(ValueError, match="independent=True is not offered"):
        M.BigEmbedStep(G, E, LP, mode="W", attention=False, independent=True)
    with pytest.raises(ValueError, match="attention=True needs the vgg16 network"):
        M.BigEmbedStep(G, E, LP, mode="W")
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **kw: 2)
    with pytest.raises(ValueError, match="more than one process is not offered"):
        M.BigEmbedStep(G, E, LP, mode="W", attention=False)
