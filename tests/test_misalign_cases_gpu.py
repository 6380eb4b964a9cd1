"""The two Cat256 mis-align iterations (dge_amd.mis_align.MisAlignStep, case="case1" | "case2") against the reference's own runs
of ablation_utils/Cat256/E_mis_align_case_1.py / E_mis_align_case_2.py's loop bodies (tests/golden/step_misalign_case{1,2}.npz,
tools/gen_golden_misalign_cases.py), the unchanged default iteration, and the refusals.

Bounds.  Masks, logged terms, the latent loss and parameters after a latent-only step: those of
tests/test_gradcam.py::test_mis_align_iteration_matches_reference_run (w2 2e-3 of its maximum, masks 5e-3 absolute, losses 5e-3
relative, info columns 1e-2 relative, sampled parameters 1e-4 of their maximum, checksum 1e-5 relative).  Parameters behind case 2's
live image phase: those of tests/test_step_gpu.py::test_two_phase_step_matches_reference_run (sampled parameters 1e-4 in the
deterministic mode and 5e-3 in the default mode, checksum 1e-5 / 1e-4)."""
import numpy as np
import pytest
import torch

from tests.conftest import MODES, golden, meas
from tests.golden import recipe as R
from tests.helpers import s2_shapes, enc_shapes
from oracle import gradcam_ref as GR
from oracle import lpips_ref as LR
from oracle import ref_torch as O

pytestmark = pytest.mark.gpu
CFG = R.GRADCAM_CFG


def _vgg():
    from dge_amd import grad_cam as G
    net = GR.VGG16Ref(CFG["widths"], CFG["fc"], CFG["classes"])
    shapes = {k: list(v.shape) for k, v in net.state_dict().items()}
    m = G.VGG16(CFG["widths"], CFG["fc"], CFG["classes"], compute_dtype="f32")
    m.load_state_dict(GR.seeded_state(shapes, CFG["seed"]))
    return m.cuda()


def _step(enc=(16, 128, 5), **kw):
    import dge_amd
    from dge_amd.encoder import BE
    from dge_amd.lpips import LPIPS
    from dge_amd.mis_align import MisAlignStep
    Gen = dge_amd.StyleGAN2Generator(64, fmaps_base=2048, fmaps_max=128, compute_dtype="f32").cuda()
    Gen.load_state_dict(R.fill_s2(s2_shapes(64, fmaps_base=2048, fmaps_max=128), seed=11))
    Gen.train()
    for p in Gen.parameters():
        p.requires_grad_(False)
    E = BE(startf=enc[0], maxf=enc[1], layer_count=enc[2], compute_dtype="f32").cuda()
    E.load_state_dict(R.fill_encoder(enc_shapes(*enc), seed=31))
    LP = LPIPS(compute_dtype="f32").cuda()
    LP.load_state_dict(LR.seeded_params(0))
    return MisAlignStep(Gen, E, LP, _vgg(), lr=0.0015, batch_size=2, **kw), E


def _inputs(it):
    z = R.randn(f"step.z{it}", (2, 512), 1)
    noises = [R.randn(f"step.it{it}.noise{i}", s, 1).cuda() for i, s in enumerate(O.enc_noise_shapes(5, 2, 64))]
    return dict(z=z, noises=noises, new_z=R.randn("step.new_z", (2, 512), 1).cuda())


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _sampled(E, g, prefix):
    """worst relative error of the sampled parameter tensors stored under `prefix` (their first `clip` elements)"""
    sd, clip, worst = E.state_dict(), int(np.asarray(g["clip"]).reshape(-1)[0]), 0.0
    keys = [k for k in g.files if k.startswith(prefix + ":")]
    assert len(keys) == 5, prefix
    for key in keys:
        worst = max(worst, rel(sd[key.split(":", 1)[1]].reshape(-1)[:clip].cpu().numpy(), g[key]))
    return worst


def _checksum_err(E, g, key):
    cs = float(np.asarray(g[key]).reshape(-1)[0])
    return abs(R.checksum({k: v.cpu() for k, v in E.state_dict().items()}) - cs) / cs


class _AfterCalls:
    """Observes the encoder after every optimizer call of an iteration (step() and, in the legacy form, tick())."""

    def __init__(self, opt, monkeypatch, fn):
        self.n = 0
        for name in ("step", "tick"):
            orig = getattr(opt, name)

            def f(*a, _orig=orig, _name=name, **kw):
                inner = getattr(self, "_in_tick", False)
                if _name == "tick":
                    self._in_tick = True
                try:
                    out = _orig(*a, **kw)
                finally:
                    if _name == "tick":
                        self._in_tick = False
                if not inner:                        # (tick() runs step() inside itself: one call)
                    self.n += 1
                    fn(self.n)
                return out
            monkeypatch.setattr(opt, name, f)


def _check_logged(r, g, pre, it, case):
    assert rel(r["w2"].cpu().numpy(), g[f"{pre}it{it}_w2"]) < 2e-3
    if not pre:
        for k in ("mask_1", "mask_2"):
            assert np.abs(r[k].cpu().numpy() - g[f"it{it}_{k}"]).max() < 5e-3, (it, k)
    ref_l = g[f"{pre}it{it}_losses"]              # imgs, mask, Gcam, grad, w, c (unweighted)
    got = [float(r["info_imgs"][0]), float(r["info_mask"][0]), float(r["info_Gcam"][0]), float(r["info_grad"][0]),
           float(r["loss_w"]), float(r["loss_c"])]
    for a, b in zip(got, ref_l):
        assert abs(a - b) < 5e-3 * abs(b), (it, got, ref_l)
    ref_info = g[f"{pre}it{it}_info"]             # rows imgs, mask, Gcam, grad, w, c; columns mse, mean, std, kl, cos, ssim, lpips
    for row, key in enumerate(("info_imgs", "info_mask", "info_Gcam", "info_grad", "info_w", "info_c")):
        info = r[key].cpu().numpy()
        for col in ((0, 4, 5, 6) if row < 4 else (0, 4)):        # (latent rows: ssim and lpips are the constant 0)
            assert abs(info[1 + col] - ref_info[row, col]) < 1e-2 * abs(ref_info[row, col]) + 1e-6, (it, key, col)
    ph = {k: float(v) for k, v in r["phase_losses"].items()}
    if case == "case2":                            # the losses stepped on: imgs, 5 * mask, 9 * Gcam, w itself
        want = dict(imgs=ref_l[0], mask=5.0 * ref_l[1], Gcam=9.0 * ref_l[2], w=ref_l[4])
    else:
        want = dict(tsa=ref_l[0] + ref_l[1] + ref_l[2], mtv=(ref_l[5] + ref_l[4]) * 0.01)
    assert ph.keys() == want.keys()
    for k in want:
        assert abs(ph[k] - want[k]) < 5e-3 * abs(want[k]), (it, k, ph, want)


def _script_calls(case, legacy, it):
    """which of the script's optimizer calls an iteration issues here, in order.  The default form skips the idle ones (no gradient:
    nothing to do); the legacy form ticks them - except case 1's very first, which only seeds the Adam states (MisAlignStep._idle_call)"""
    if case == "case2":
        return [1, 2, 3, 4] if legacy else [1, 4]
    return [1, 2] if (legacy and it > 0) else [2]


def _run_case(case, attention, mode, legacy, monkeypatch):
    from dge_amd import ops
    assert ops.is_deterministic() == (mode == "det")
    g = golden("step_misalign_%s.npz" % case)
    assert tuple(g["encoder"]) == (16, 128, 5)
    pre = "legacy_" if legacy else ""
    st, E = _step(case=case, attention=attention, zero_grad_to_none=not legacy)
    # (sampled parameters, checksum): behind a step on the live image gradient (case 2) / behind latent-only steps (case 1)
    bound = ((1e-4, 1e-5) if mode == "det" else (5e-3, 1e-4)) if case == "case2" else (1e-4, 1e-5)
    seen = []

    def after(n):
        key = f"{pre}it{it}_call{_script_calls(case, legacy, it)[n - 1]}"
        has = any(k.startswith(key + ":") for k in g.files)
        seen.append((key, _checksum_err(E, g, key + "_checksum"), _sampled(E, g, key) if has else None))
    calls = _AfterCalls(st.opt, monkeypatch, after)
    for it in range(2):
        del seen[:]
        calls.n = 0
        r = st.step(it, **_inputs(it))
        _check_logged(r, g, pre, it, case)
        assert calls.n == len(_script_calls(case, legacy, it)), (it, calls.n)
        meas(f"misalign_{case}_{attention}_{mode}_{pre}it{it}", **{k.split("_")[-1] + "_checksum": c for k, c, _ in seen},
             **{k.split("_")[-1] + "_sampled": v for k, _, v in seen if v is not None})
        for key, cs, smp in seen:
            assert cs < bound[1], (key, cs)
            assert smp is None or smp < bound[0], (key, smp)
        assert seen[-1][2] is not None                  # the iteration's last call carries the sampled tensors
    return st, E, g


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("attention", ["pair", "fused"])
@pytest.mark.parametrize("case", ["case1", "case2"])
def test_cat256_iterations_match_reference_run(case, attention, mode, monkeypatch):
    _run_case(case, attention, mode, False, monkeypatch)


@pytest.mark.parametrize("case", ["case1", "case2"])
def test_cat256_legacy_zero_grad_matches_reference_run(case, monkeypatch):
    """zero_grad(set_to_none=False): case 2's two idle optimizer calls tick the Adam states between the image and the latent step;
    case 1's idle call does from the first iteration on.  The default form must NOT reproduce these arrays."""
    st, E, g = _run_case(case, "pair", "det", True, monkeypatch)
    last = 4 if case == "case2" else 2
    st2, E2 = _step(case=case, attention="pair")
    for it in range(2):
        st2.step(it, **_inputs(it))
    assert _sampled(E2, g, f"it1_call{last}") < 1e-4                     # the default form is on its own arrays ...
    assert _sampled(E2, g, f"legacy_it1_call{last}") > 1e-4              # ... and off the legacy ones by more than the bound
    assert _sampled(E, g, f"it1_call{last}") > 1e-4


def _s1_step_as_before(st, iteration, z, noises, new_z):
    """MisAlignStep.step as it stood before the Cat256 cases were added (fused attention), restated"""
    from dge_amd import losses, ops
    from dge_amd.grad_cam import mask2cam
    z, imgs1, w1, const2, w2, imgs2 = st._head(iteration, z, noises, (None, None), new_z, synth_grad=False)
    with torch.no_grad():
        mask_1, grad_1 = st.grad_cam_plus_plus.with_input_gradient(imgs1)
        mask_2, grad_2 = st.grad_cam_plus_plus.with_input_gradient(imgs2)
        heat_1, cam_1 = mask2cam(mask_1, imgs1)
        heat_2, cam_2 = mask2cam(mask_2, imgs2)
        _, info_grad = losses.space_loss(grad_1, grad_2, lpips_model=st.lpips, global_batch=None)
        l_imgs, info_imgs = losses.space_loss(imgs1, imgs2, lpips_model=st.lpips, global_batch=None)
        l_mask, info_mask = losses.space_loss(mask_1, mask_2, lpips_model=st.lpips, global_batch=None)
        l_cam, info_cam = losses.space_loss(cam_1, cam_2, lpips_model=st.lpips, global_batch=None)
        loss_tsa = l_imgs + l_mask + l_cam
    loss_w, info_w = losses.space_loss(w1, w2, image_space=False, global_batch=None)
    loss_mtv = loss_w * 0.01
    st.opt.zero_grad()
    loss_mtv.backward()
    st.opt.step(grad_scale=None)
    ops.zero_arena_end()
    return dict(w2=w2.detach(), mask_1=mask_1, mask_2=mask_2, cam_2=cam_2, grad_2=grad_2, loss_tsa=loss_tsa, loss_w=loss_w.detach())


def test_default_s1_iteration_issues_the_launches_it_issued_before():
    from dge_amd import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        runs = []
        for fn in ("step", "before"):
            st, E = _step(enc=(16, 64, 5))                  # no keyword: case "s1", fused attention
            assert (st.case, st.attention, st.fused_attention) == ("s1", "fused", True)
            logs, outs = [], []
            for it in range(2):
                ops.KERNEL_LOG = log = []
                try:
                    r = st.step(it, **_inputs(it)) if fn == "step" else _s1_step_as_before(st, it, **_inputs(it))
                finally:
                    ops.KERNEL_LOG = None
                logs.append([n for n, _ in log])
                outs.append(r)
            torch.cuda.synchronize()
            runs.append((logs, outs, {k: v.clone() for k, v in E.state_dict().items()}))
    finally:
        ops.set_deterministic(was)
    (logs_a, outs_a, sd_a), (logs_b, outs_b, sd_b) = runs
    assert logs_a == logs_b and len(logs_a[0]) > 20
    assert not any("groups" in n for n in logs_a[0]) and logs_a[0].count("class_target") == 2 and logs_a[0].count("mask2cam") == 2
    for ra, rb in zip(outs_a, outs_b):
        for k in rb:
            assert torch.equal(ra[k], rb[k]), k
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k
    assert outs_a[0]["info_c"] is None and set(outs_a[0]["phase_losses"]) == {"tsa", "mtv"}


def test_pair_attention_s1_iteration_matches_reference_run():
    """the third routing on the iteration that has a fixture of its own (step_misalign.npz, the bounds of test_gradcam.py's test)"""
    g = golden("step_misalign.npz")
    st, E = _step(enc=(16, 64, 5), attention="pair")
    for it in range(2):
        ops_log = []
        from dge_amd import ops
        ops.KERNEL_LOG = ops_log
        try:
            r = st.step(it, **_inputs(it))
        finally:
            ops.KERNEL_LOG = None
        names = [n for n, _ in ops_log]
        assert names.count("class_target_groups") == 1 and names.count("mask2cam_groups") == 1 and "mask2cam" not in names
        for k in ("mask_1", "mask_2"):
            assert np.abs(r[k].cpu().numpy() - g[f"it{it}_{k}"]).max() < 5e-3, (it, k)
        got = [float(r["loss_tsa"]), float(r["info_imgs"][0]), float(r["info_mask"][0]), float(r["info_Gcam"][0]),
               float(r["info_grad"][0]), float(r["loss_w"])]
        for a, b in zip(got, g[f"it{it}_losses"]):
            assert abs(a - b) < 5e-3 * abs(b), (it, got)
        cs = float(np.asarray(g[f"it{it}_param_checksum"]).reshape(-1)[0])
        assert abs(R.checksum({k: v.cpu() for k, v in E.state_dict().items()}) - cs) < 1e-5 * cs


def test_refusals_raise_with_their_messages():
    import dge_amd
    from dge_amd import mis_align as M
    from dge_amd.models import build_models_pg
    st, _ = _step(case="case2")
    with pytest.raises(RuntimeError, match="capture is not offered for case2"):
        st.capture()
    with pytest.raises(ValueError, match="prefetch_next is not offered"):
        st.step(0, prefetch_next=True)
    with pytest.raises(ValueError, match="case must be one of"):
        _step(case="case3")
    with pytest.raises(ValueError, match="attention must be one of"):
        _step(attention="both")
    G, E, LP = build_models_pg(64, 16, "f32", lpips=True)
    for case in ("case1", "case2"):
        with pytest.raises(ValueError, match="loss_c is not meaningful"):
            M.MisAlignStep(G, E, LP, _vgg(), case=case)
    st, _ = _step(enc=(16, 64, 5), case="case1")          # const1 [2,128,4,4] against const2 [2,64,4,4]
    with pytest.raises(ValueError, match="differ in shape"):
        st.step(0, **_inputs(0))
    st, _ = _step(enc=(16, 64, 5), case="case2")          # case 2 only logs loss_c: it is left out
    r = st.step(0, **_inputs(0))
    assert r["loss_c"] is None and r["info_c"] is None and set(r["phase_losses"]) == {"imgs", "mask", "Gcam", "w"}
