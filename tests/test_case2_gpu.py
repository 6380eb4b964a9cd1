"""Per-loss-update encoder training (dge_amd.e_align_case2): the split window-gradient kernel against the single-window kernel,
the merged one and the CPU oracle, and Case2Step against the reference's own runs of ablation_utils/8.E_align_x_AT1_AT2.py,
6.E_align_x.py and Cat256/E_align_case_2.py at reduced size (tools/gen_golden.py sections step_case2_sg1 / _sub / _s2).

Bounds of the step parity: those tests/test_step_gpu.py applies to the same quantities of the two-step loop (w1 1e-4, imgs1 5e-4,
w2 / imgs2 2e-3, losses 2e-3 relative, parameters 1e-4 deterministic / 5e-3 atomics, first-iteration update 0.05), each widened to
4 x the reference's own f32-vs-f64 spread of that quantity where that is larger (`*_ref_spread` in the goldens).  The stored
spreads are 5e-9 .. 1.2e-5 (largest: a conv weight after the third optimizer step of the subset run), so 4 x spread never
exceeds a project bound and the effective bounds are the project's."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.conftest import golden, meas, MODES
from tests.golden import recipe as R
from tests.helpers import s2_shapes
from oracle import ref_torch as O
from oracle import lpips_ref as LR

pytestmark = pytest.mark.gpu


def relerr(a, b):
    a = a.detach().float().cpu()
    b = torch.as_tensor(np.asarray(b)).float()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


# ----------------------------------------------------------------------------------------------------------------- kernel
def _split_case(B, Cc, H, W, wins, ks):
    from dge_amd._lib import lib, check
    L = lib()
    dev = "cuda"
    a = R.randn("c2k.a", (B, Cc, H, W), 5, 0.5).cuda()
    b = (a * 0.8 + R.randn("c2k.b", (B, Cc, H, W), 6, 0.2).cuda()).contiguous()
    nw = len(wins)
    wts = [1.0, 5.0, 9.0][:nw]
    sums, gps, ns = [], [], []
    for i, (y0, x0, h, w) in enumerate(wins):
        ca, cb = a[:, :, y0:y0 + h, x0:x0 + w].double(), b[:, :, y0:y0 + h, x0:x0 + w].double()
        s = torch.zeros(8, dtype=torch.float64)
        s[0], s[1], s[2], s[3], s[4], s[5] = ((ca - cb) ** 2).sum(), (ca * cb).sum(), (ca * ca).sum(), (cb * cb).sum(), ca.sum(), cb.sum()
        sums.append(s.float().cuda())
        gps.append(R.randn(f"c2k.gp{i}", (B, Cc, h // ks[i], w // ks[i]), 7, 1e-3).cuda())
        ns.append(float(B * Cc * h * w))
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda ts: (C.c_void_p * nw)(*[t.data_ptr() for t in ts])
    wflat = (C.c_int * (4 * nw))(*[int(v) for win in wins for v in win])
    kk, nn, ww = (C.c_int * nw)(*ks), (C.c_float * nw)(*ns), (C.c_float * nw)(*wts)
    outs = [torch.full((B, Cc, H, W), float("nan"), device=dev) for _ in range(nw)]        # every element must be written
    check(L.dge_space_loss_bwd_split(a.data_ptr(), b.data_ptr(), ptr(sums), ptr(gps), ptr(outs), B * Cc, H, W, wflat, kk, nn, ww, nw, st),
          "dge_space_loss_bwd_split")
    name = L.dge_last_kernel().decode()
    refs = []
    for i, (y0, x0, h, w) in enumerate(wins):
        z = torch.zeros((B, Cc, H, W), device=dev)
        check(L.dge_space_loss_bwd(a.data_ptr(), b.data_ptr(), sums[i].data_ptr(), gps[i].data_ptr(), z.data_ptr(), B * Cc, H, W, y0, x0, h, w,
                                   ks[i], ns[i], wts[i], 0, st), "dge_space_loss_bwd")
        refs.append(z)
    g3 = torch.zeros((B, Cc, H, W), device=dev)
    check(L.dge_space_loss_bwd3(a.data_ptr(), b.data_ptr(), ptr(sums), ptr(gps), g3.data_ptr(), B * Cc, H, W, wflat, kk, nn, ww, nw, st),
          "dge_space_loss_bwd3")
    return outs, refs, g3, name


def _wins(H, W):
    from dge_amd.losses import attention_windows
    return attention_windows(H, W)


@pytest.mark.parametrize("B,Cc,H,W,ks", [(2, 3, 64, 64, (1, 1, 1)), (1, 3, 256, 256, (1, 1, 1)), (2, 3, 44, 30, (1, 1, 1)),
                                         (1, 2, 37, 53, (1, 1, 1)), (2, 3, 64, 64, (2, 2, 2)), (1, 3, 512, 512, (2, 2, 1))])
def test_split_kernel_equals_single_window_kernel_and_sums_to_merged_kernel(B, Cc, H, W, ks):
    """Output k of dge_space_loss_bwd_split against dge_space_loss_bwd for window k on a zeroed image: the per-element expression is
    the same source, term by term, but it is compiled into a different kernel, where the compiler is free to contract a multiply
    and an add into an FMA differently - so the bound is 1e-6 of max|ref| (a few f32 ulps of the largest element), and the measured
    difference is printed.  The sum over k against dge_space_loss_bwd3 (reciprocal-multiply arithmetic): 1e-6 of the max too."""
    wins = _wins(H, W)
    assert all(win[2] % k == 0 and win[3] % k == 0 for win, k in zip(wins, ks))
    outs, refs, g3, name = _split_case(B, Cc, H, W, wins, list(ks))
    assert name == ("space_loss_bwd_split_v4" if W % 4 == 0 else "space_loss_bwd_split"), name
    worst, exact = 0.0, True
    for k, (o, r) in enumerate(zip(outs, refs)):
        assert torch.isfinite(o).all(), k
        y0, x0, h, w = wins[k]
        outside = o.clone()
        outside[:, :, y0:y0 + h, x0:x0 + w] = 0
        assert float(outside.abs().max()) == 0.0, k                      # zeros outside the window, written not left over
        e = ((o - r).abs().max() / r.abs().max()).item()
        worst, exact = max(worst, e), exact and torch.equal(o, r)
        assert e <= 1e-6, (k, e)
    tot = outs[0] + outs[1] + outs[2]
    e3 = ((tot - g3).abs().max() / g3.abs().max()).item()
    meas("case2_split_kernel", B=B, H=H, W=W, k0=ks[0], worst=worst, bit_exact=float(exact), sum_vs_bwd3=e3)
    assert e3 <= 1e-6, e3


def test_split_kernel_skips_zero_weight_and_null_outputs():
    from dge_amd._lib import lib, check
    L = lib()
    B, Cc, H, W = 1, 3, 64, 64
    wins = _wins(H, W)
    a = R.randn("c2k.a", (B, Cc, H, W), 5, 0.5).cuda()
    b = R.randn("c2k.b", (B, Cc, H, W), 6, 0.5).cuda()
    sums = [torch.ones(8, device="cuda") for _ in range(3)]
    outs = [torch.full((B, Cc, H, W), 7.0, device="cuda") for _ in range(3)]
    ptr = lambda ts: (C.c_void_p * 3)(*[(t.data_ptr() if t is not None else None) for t in ts])
    wflat = (C.c_int * 12)(*[int(v) for win in wins for v in win])
    check(L.dge_space_loss_bwd_split(a.data_ptr(), b.data_ptr(), ptr(sums), None, ptr([outs[0], None, outs[2]]), B * Cc, H, W, wflat,
                                     (C.c_int * 3)(1, 1, 1), (C.c_float * 3)(1.0, 1.0, 1.0), (C.c_float * 3)(1.0, 5.0, 0.0), 3,
                                     torch.cuda.current_stream().cuda_stream), "dge_space_loss_bwd_split")
    assert float((outs[0] - 7.0).abs().max()) > 0                        # written
    assert torch.equal(outs[1], torch.full_like(outs[1], 7.0))           # null pointer: skipped (not passed at all)
    assert torch.equal(outs[2], torch.full_like(outs[2], 7.0))           # weight 0: skipped


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("B,H,W", [(1, 512, 512), (2, 44, 30)])
def test_split_losses_and_gradients_vs_oracle(B, H, W, det):
    """Each of the three losses and ITS gradient against the oracle's autograd on that crop alone (the 2e-3-of-max bound of
    tests/test_loss_gpu.py), in both reduction modes; a window switched off keeps its info row and has no gradient."""
    from dge_amd import losses, ops
    a = R.randn("tsa.a", (B, 3, H, W), 3, 0.4)
    b0 = a * 0.8 + R.randn("tsa.b", (B, 3, H, W), 3, 0.2)
    zero_lp = lambda x, y: torch.zeros(x.shape[0], 1, 1, 1)
    was = ops.is_deterministic()
    ops.set_deterministic(det)
    try:
        bg = b0.cuda().requires_grad_(True)
        ls, info = losses.image_losses_split(a.cuda(), bg)
        assert tuple(info.shape) == (3, 8)
        for k, wgt in enumerate((1, 5, 9)):
            b = b0.clone().requires_grad_(True)
            x1, x2 = [a, *O.attention_crops(a)][k], [b, *O.attention_crops(b)][k]
            l, _ = O.space_loss(x1, x2, lpips_fn=zero_lp)
            (wgt * l).backward()
            bg.grad = None
            ls[k].backward(retain_graph=True)
            assert abs(float(ls[k]) - wgt * float(l)) < 2e-4 * abs(wgt * float(l)), k
            err = ((bg.grad.cpu() - b.grad).abs().max() / b.grad.abs().max()).item()
            meas("case2_split_vs_oracle", B=B, H=H, k=k, det=float(det), err=err)
            assert err < 2e-3, (k, err)
        bg2 = b0.cuda().requires_grad_(True)
        ls2, info2 = losses.image_losses_split(a.cuda(), bg2, windows=(True, False, True))
        assert not ls2[1].requires_grad and ls2[0].requires_grad and ls2[2].requires_grad
        assert torch.allclose(info2, info, rtol=1e-5, atol=1e-7)
    finally:
        ops.set_deterministic(was)


# ----------------------------------------------------------------------------------------------------------------- step
def _blur_shapes(E):
    return {k: list(v.shape) for k, v in E.state_dict().items()}


def _encoder():
    from dge_amd.encoder_variants import BlurBE
    E = BlurBE(startf=16, maxf=64, layer_count=5, compute_dtype="f32").cuda()
    sd = R.fill_encoder(_blur_shapes(E), seed=31)
    for k in sd:
        if k.endswith("blur.weight"):
            sd[k] = E.state_dict()[k].clone()
    E.load_state_dict(sd)
    return E, {k: v.clone() for k, v in sd.items()}


def _lpips():
    from dge_amd.lpips import LPIPS
    LP = LPIPS(compute_dtype="f32").cuda()
    LP.load_state_dict(LR.seeded_params(0))
    return LP


def _sg1_models():
    import dge_amd.stylegan1 as S
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
    return Gs, Gm


def _s2_model():
    import dge_amd
    G = dge_amd.StyleGAN2Generator(64, fmaps_base=2048, fmaps_max=128, compute_dtype="f32").cuda()
    G.load_state_dict(R.fill_s2(s2_shapes(64, fmaps_base=2048, fmaps_max=128), seed=11))
    G.train()
    for p in G.parameters():
        p.requires_grad_(False)
    return G


def _tol(g, key, project):
    """max(project tolerance, 4 x the reference's own f32-vs-f64 spread of the stored quantity)"""
    return max(project, 4.0 * float(g[key + "_ref_spread"]))


class _PhaseTap:
    """Records the encoder parameters after every optimizer step of an iteration (LREQAdam.step wrapped on the instance)."""

    def __init__(self, st, keys):
        self.snaps, self.st, self.keys = [], st, keys
        inner = st.opt.step

        def step(*a, **k):
            r = inner(*a, **k)
            sd = st.E.state_dict()
            self.snaps.append({key: sd[key].detach().clone() for key in keys})
            return r
        st.opt.step = step


def _head(t, ref):
    t = t.detach().cpu()
    return t.flatten()[:ref.size] if t.numel() > ref.size else t.reshape(ref.shape)


def _check_params(g, it, tap, before, mode, nphase, kind):
    assert len(tap.snaps) == nphase, len(tap.snaps)
    for ph in range(1, nphase + 1):
        for key in [k for k in g.files if k.startswith(f"it{it}_after_phase{ph}:") and not k.endswith("_ref_spread")]:
            k = key.split(":", 1)[1]
            ref = g[key]
            mine = _head(tap.snaps[ph - 1][k], ref)
            e = relerr(mine, ref)
            meas("case2_param", it=it, phase=ph, key=k, mode=mode, err=e)
            assert e < _tol(g, key, 1e-4 if mode == "det" else 5e-3), (it, ph, k, e)
            if it == 0:
                # the UPDATE of this optimizer step, not the value (a step moves a parameter by ~lr * coef).  StyleGAN2 in the
                # deterministic mode: largest element, as test_two_phase_step_matches_reference_run; otherwise in the L2 sense, as
                # the StyleGAN1 and atomics-mode cases there (with beta1 = 0 the first steps are sign-like: an element whose
                # gradient is within rounding of zero may step the other way)
                prev_ref = _head(before[k], ref) if ph == 1 else torch.as_tensor(g[f"it0_after_phase{ph - 1}:{k}"]).float()
                prev = _head(before[k], ref) if ph == 1 else _head(tap.snaps[ph - 2][k], ref)
                du_ref, du = torch.as_tensor(ref).float() - prev_ref, mine - prev
                if du_ref.abs().max() > 0:
                    d = (((du - du_ref).abs().max() / du_ref.abs().max()).item() if (mode == "det" and kind == "s2")
                         else ((du - du_ref).norm() / du_ref.norm()).item())
                    meas("case2_update", phase=ph, key=k, mode=mode, kind=kind, err=d)
                    assert d < 0.05, (ph, k, d)


def _run_parity(kind, mode, gname, image_phases, latent_terms, latent_scale, full=True):
    from dge_amd import ops
    from dge_amd.e_align_case2 import Case2Step
    assert ops.is_deterministic() == (mode == "det")
    g = golden(gname)
    E, before = _encoder()
    keys = sorted({k.split(":", 1)[1] for k in g.files if ":" in k and not k.endswith("_ref_spread")})
    if kind == "sg1":
        Gs, Gm = _sg1_models()
        st = Case2Step(Gs, E, _lpips(), mapping=Gm, image_phases=image_phases, latent_terms=latent_terms, latent_scale=latent_scale,
                       lr=0.0015, batch_size=2)
    else:
        st = Case2Step(_s2_model(), E, _lpips(), image_phases=image_phases, latent_terms=latent_terms, latent_scale=latent_scale,
                       lr=0.0015, batch_size=2)
    tap = _PhaseTap(st, keys)
    nshapes = [tuple(int(v) for v in s if v) for s in g["noise_shapes"].tolist()]
    n_first, n_enc = [int(v) for v in g["noise_split"]]
    nphase = len(image_phases) + 1
    pfx = "c2sg1" if kind == "sg1" else "c2s2"
    new_z = R.randn("step.new_z", (2, 512), 1).cuda()
    for it in range(2):
        tap.snaps.clear()
        nz = [R.randn(f"{pfx}.it{it}.noise{i}", s, 1) for i, s in enumerate(nshapes)]
        enc_nz = [n.cuda() for n in nz[n_first:n_first + n_enc]]
        if kind == "sg1":
            r = st.step(it, z=R.randn(f"sg1step.z{it}", (2, 512), 1), noises=enc_nz, gen_noises=(nz[:n_first], nz[n_first + n_enc:]))
        else:
            np.random.seed(it)
            r = st.step(it, z=R.randn(f"step.z{it}", (2, 512), 1), noises=enc_nz, new_z=new_z)
        if full:
            errs = {k: relerr(r[k], g[f"it{it}_{k}"]) for k in ("w1", "imgs1", "w2", "imgs2", "const2")}
            meas("case2_step_" + kind, it=it, mode=mode, **errs)
            assert errs["w1"] < _tol(g, f"it{it}_w1", 1e-4) and errs["imgs1"] < _tol(g, f"it{it}_imgs1", 5e-4), errs
            assert errs["w2"] < _tol(g, f"it{it}_w2", 2e-3) and errs["imgs2"] < _tol(g, f"it{it}_imgs2", 2e-3), errs
            assert errs["const2"] < _tol(g, f"it{it}_const2", 2e-3), errs
            info, ref_info = r["info_img"].cpu().numpy(), g[f"it{it}_info"]
            for row in range(3):
                for col in (0, 4, 5, 6):            # mse, cos, ssim, lpips (as tests/test_step_gpu.py)
                    assert abs(info[row, 1 + col] - ref_info[row, col]) < 3e-3 * abs(ref_info[row, col]) + 1e-6, (it, row, col)
        ref_l = g[f"it{it}_losses"]          # imgs, 5*AT1, 9*AT2, w, c, mslv
        got = [float(r["loss_imgs"]), float(r["loss_medium"]), float(r["loss_small"]), float(r["loss_w"]),
               float(r["loss_c"]) if r["loss_c"] is not None else 0.0, float(r["loss_mslv"])]
        ltol = _tol(g, f"it{it}_losses", 2e-3)
        meas("case2_losses_" + kind, it=it, mode=mode, worst=max(abs(a - b) / abs(b) for a, b in zip(got, ref_l) if b != 0))
        for a, b in zip(got, ref_l):
            assert abs(a - b) <= ltol * abs(b), (it, got, ref_l)
        _check_params(g, it, tap, before, mode, nphase, kind)
        cs = float(g[f"it{it}_param_checksum"])
        assert abs(R.checksum({k: v.cpu() for k, v in E.state_dict().items()}) - cs) < (1e-5 if mode == "det" else 1e-4) * cs
        if it == 0:
            # separation is real: every optimizer step moved the encoder
            prev = before
            for ph, snap in enumerate(tap.snaps):
                assert any(not torch.equal(snap[k].cpu(), prev[k].cpu()) for k in keys), ph
                prev = snap
    # LREQAdam was called once per requested phase and iteration (a phase left out makes no optimizer call)
    steps = {st_["step"] for st_ in st.opt.state.values() if len(st_)}
    assert max(steps) == 2 * nphase, steps
    return st


@pytest.mark.parametrize("mode", MODES)
def test_case2_step_stylegan1_matches_reference_run(mode):
    """ablation 8 (imgs, AT1, AT2 steps, then (loss_w + loss_c) * 0.01): parameters compared after EVERY optimizer step."""
    _run_parity("sg1", mode, "step_case2_sg1.npz", ("imgs", "AT1", "AT2"), ("w", "c"), 0.01)


@pytest.mark.parametrize("mode", MODES)
def test_case2_step_stylegan2_matches_reference_run(mode):
    """Cat256/E_align_case_2.py --mtype 2 (train-mode generator, injected style-mixing latent), last step on loss_w unscaled."""
    _run_parity("s2", mode, "step_case2_s2.npz", ("imgs", "AT1", "AT2"), ("w",), 1.0)


@pytest.mark.parametrize("mode", MODES)
def test_case2_subset_matches_reference_run(mode):
    """ablation 6: the image step and the latent step only - two LREQAdam calls per iteration, not four."""
    st = _run_parity("sg1", mode, "step_case2_sub.npz", ("imgs",), ("w", "c"), 0.01, full=False)
    assert max(s["step"] for s in st.opt.state.values() if len(s)) == 4


def test_second_phase_backward_reads_the_weights_of_the_first_step():
    """Q3: the AT1 update of the full ladder differs from the AT1 update of a run whose only image phase is AT1 (same inputs, same
    gradient image): the second backward saw the weights phase 1 left."""
    from dge_amd import ops
    from dge_amd.e_align_case2 import Case2Step
    g = golden("step_case2_sg1.npz")
    nshapes = [tuple(int(v) for v in s if v) for s in g["noise_shapes"].tolist()]
    n_first, n_enc = [int(v) for v in g["noise_split"]]
    key = "decode_block.3.conv_2.weight"
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        upd = []
        for phases in (("imgs", "AT1", "AT2"), ("AT1",)):
            E, before = _encoder()
            Gs, Gm = _sg1_models()
            st = Case2Step(Gs, E, _lpips(), mapping=Gm, image_phases=phases, lr=0.0015, batch_size=2)
            tap = _PhaseTap(st, [key])
            nz = [R.randn(f"c2sg1.it0.noise{i}", s, 1) for i, s in enumerate(nshapes)]
            st.step(0, z=R.randn("sg1step.z0", (2, 512), 1), noises=[n.cuda() for n in nz[n_first:n_first + n_enc]],
                    gen_noises=(nz[:n_first], nz[n_first + n_enc:]))
            i = phases.index("AT1")
            prev = tap.snaps[i - 1][key] if i else before[key].cuda()
            upd.append((tap.snaps[i][key] - prev).cpu())
        d = ((upd[0] - upd[1]).norm() / upd[1].norm()).item()
        meas("case2_q3", diff=d)
        assert d > 1e-3, d
    finally:
        ops.set_deterministic(was)


def test_capture_is_not_offered():
    from dge_amd.e_align_case2 import Case2Step
    Gs, Gm = _sg1_models()
    E, _ = _encoder()
    st = Case2Step(Gs, E, None, mapping=Gm)
    with pytest.raises(RuntimeError, match="eager"):
        st.capture()
    with pytest.raises(ValueError, match="prefetch_next"):
        st.step(0, prefetch_next=True)


@pytest.mark.parametrize("mtype,size,startf", [(1, 256, 64), (2, 1024, 16)])
def test_fullsize_bf16_case2_step_runs_and_trains(mtype, size, startf):
    """One bf16 iteration at StyleGAN1-256 / E_Blur(64, 7 blocks) and StyleGAN2-1024 / E_Blur(16, 9 blocks), batch 2, seeded
    weights: finite results, every encoder parameter that received a gradient moved, the split loss kernel ran once.  No parity
    is claimed at this size."""
    from dge_amd import ops
    from dge_amd.e_align_case2 import Case2Step, build_models
    G, Gm, E, LP = build_models(mtype, size, startf, "bf16")
    assert E.layer_count == (7 if mtype == 1 else 9)
    st = Case2Step(G, E, LP, mapping=Gm, latent_terms=("w", "c") if mtype == 1 else ("w",), latent_scale=0.01 if mtype == 1 else 1.0,
                   batch_size=2)
    before = {k: v.detach().clone() for k, v in E.named_parameters()}
    ops.KERNEL_LOG = []
    try:
        r = st.step(0)
        log = [n for n, _ in ops.KERNEL_LOG]
    finally:
        ops.KERNEL_LOG = None
    assert log.count("space_loss_bwd_split_v4") == 1 and not any(n == "space_loss_bwd_split" for n in log), log[-5:]
    assert tuple(r["imgs2"].shape) == (2, 3, size, size)
    for k in ("imgs1", "imgs2", "w1", "w2", "const2", "info_img", "loss_imgs", "loss_medium", "loss_small", "loss_w", "loss_mslv", "info_w"):
        assert torch.isfinite(r[k].float()).all(), k
    if mtype == 1:
        assert torch.isfinite(r["loss_c"]).all() and torch.isfinite(r["info_c"]).all()
    moved = 0
    for k, p in E.named_parameters():
        if p.grad is not None and float(p.grad.abs().max()) > 0:
            assert not torch.equal(p.detach(), before[k]), k
            moved += 1
    assert moved >= 50, moved
