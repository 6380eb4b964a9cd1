"""Inversion loop of the reference's v2 scripts (embedding_v2_styleGAN1.py / embedding_v2_styleGAN2.py) on the HIP path
(dge_amd.embedding_v2): the four cases StyleGAN1 / StyleGAN2 x encoder fine-tuning / W+ optimisation against two iterations of
the reference's own modules (tests/golden/embed_v2.npz, tools/gen_golden.py `embed_v2`), the latent p-norm kernel, the
device-side trackers against a host restatement of the reference's `if` chains, the frozen-encoder backward, graph replay, and
the full-size StyleGAN2-1024 loop."""
import numpy as np
import pytest
import torch

from tests.conftest import MODES, golden, meas
from tests.golden import recipe as R
from oracle import lpips_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [("sg1", "E"), ("sg1", "W"), ("sg2", "E"), ("sg2", "W")]


def relerr(a, b):
    a = a.detach().float().cpu()
    b = torch.as_tensor(np.asarray(b)).float()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def l2rel(a, b):
    a = a.detach().float().cpu().flatten(); b = torch.as_tensor(np.asarray(b)).float().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def make_models(gen, cd="f32"):
    import dge_amd
    import dge_amd.stylegan1 as S
    from dge_amd.encoder_variants import BlurBE
    from dge_amd.lpips import LPIPS
    from tests.helpers import s2_shapes
    L = 5
    if gen == "sg1":
        from tests.test_sg1 import sg1_shapes
        G = S.Generator(startf=16, maxf=64, layer_count=L, latent_size=512, compute_dtype=cd).cuda()
        shapes = sg1_shapes(16, 64, L)
        sd = R.fill_encoder(shapes, seed=43)
        blur = torch.tensor([[1., 2., 1.], [2., 4., 2.], [1., 2., 1.]]) / 16.0
        for k in sd:
            if k.endswith("blur.weight"):
                sd[k] = blur.view(1, 1, 3, 3).repeat(shapes[k][0], 1, 1, 1)
        sd["const"] = R.randn("sg1step.const", tuple(shapes["const"]), 43)
        G.load_state_dict(sd)
    else:
        G = dge_amd.StyleGAN2Generator(64, fmaps_base=2048, fmaps_max=128, compute_dtype=cd).cuda()
        G.load_state_dict(R.fill_s2(s2_shapes(64, fmaps_base=2048, fmaps_max=128), seed=11))
        G.eval()
    for p in G.parameters():
        p.requires_grad_(False)
    E = BlurBE(startf=16, maxf=64, layer_count=L, compute_dtype=cd).cuda()
    esd = R.fill_encoder({k: list(v.shape) for k, v in E.state_dict().items()}, seed=71)
    for k in esd:
        if k.endswith("blur.weight"):
            esd[k] = E.state_dict()[k].clone()
    E.load_state_dict(esd)
    LP = LPIPS(compute_dtype=cd).cuda()
    LP.load_state_dict(LR.seeded_params(0))
    return G, E, LP


def case_noises(g, tag, it):
    """(E(imgs1), G, E(imgs2)) noise lists of iteration `it` of a golden case (G's on the host, as EmbedStep's parity test)."""
    shapes = [tuple(s) for s in g[f"{tag}_noise_shapes"].tolist()]
    s0, s1, s2 = [int(v) for v in g[f"{tag}_noise_split"].tolist()]
    nz = [R.randn(f"embed_v2.{tag}.it{it}.noise{i}", s, 2) for i, s in enumerate(shapes)]
    return ([n.cuda() for n in nz[:s0]] or None, nz[s0:s1] or None, [n.cuda() for n in nz[s1:s2]])


def begin(st, g, gen, mode, imgs1):
    tag = f"{gen}_{mode}"
    if mode == "W" and gen == "sg1":
        shapes = [tuple(s) for s in g[f"{tag}_init_noise_shapes"].tolist()]
        st.begin_image(imgs1, noises=[R.randn(f"embed_v2.{tag}.init.noise{i}", s, 2).cuda() for i, s in enumerate(shapes)])
    elif mode == "W":
        st.begin_image(imgs1, w_init=torch.as_tensor(g[f"{tag}_w0"]))
    else:
        st.begin_image(imgs1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gen,opt", CASES)
def test_embed_v2_loop_matches_reference_run(gen, opt, mode):
    from dge_amd.embedding_v2 import LatentEmbedStep
    g = golden("embed_v2.npz")
    tag = f"{gen}_{opt}"
    G, E, LP = make_models(gen)
    st = LatentEmbedStep(G, E, LP, mode=opt, generator=gen, lr=0.005)
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    begin(st, g, gen, opt, imgs1)
    if opt == "W":
        assert relerr(st.w1, g[f"{tag}_w0"]) < 1e-3
    lt = 1e-3 if mode == "det" else 3e-3
    pnames = ["decode_block.0.conv_1.weight", "decode_block.2.inver_mod1.bias", "FromRGB.from_rgb.weight"]
    for it in range(2):
        calls = []
        orig = st.opt.step

        def spy(*a, **kw):
            if opt == "E":
                calls.append({k: p.grad.detach().clone() for k, p in E.named_parameters() if k in pnames})
            else:
                calls.append({"w1": st.w1.grad.detach().clone()})
            return orig(*a, **kw)
        st.opt.step = spy
        try:
            r = st.step(imgs1, noises=case_noises(g, tag, it))
        finally:
            st.opt.step = orig
        pre = f"{tag}_it{it}"
        e_w1 = relerr(r["w1"], g[f"{pre}_w1"])
        meas(f"embed_v2.{tag}.{mode}.it{it}", w1=e_w1, w1_l2=l2rel(r["w1"], g[f"{pre}_w1"]), w2=relerr(r["w2"], g[f"{pre}_w2"]))
        if opt == "W":
            # a W-mode w1 has taken 4 sign-like Adam steps (lr 0.005): an element whose gradient is within rounding of 0 may
            # step the other way (2*lr against max|w1| ~ 4)
            assert l2rel(r["w1"], g[f"{pre}_w1"]) < 1e-3 and e_w1 < 4e-3, (it, e_w1)
        else:
            assert e_w1 < 1e-3, (it, e_w1)
        assert relerr(r["w2"], g[f"{pre}_w2"]) < (2e-3 if it == 0 else 1e-2), it
        if f"{pre}_imgs2" in g.files:
            assert relerr(r["imgs2"], g[f"{pre}_imgs2"]) < 2e-3
        assert relerr(r["const3"], g[f"{pre}_const3"]) < (2e-3 if it == 0 else 1e-2)
        if f"{pre}_const2" in g.files:
            assert relerr(r["const2"], g[f"{pre}_const2"]) < 1e-3
        else:
            assert r["const2"] is None and r["loss_c1"] is None
        info = r["info_img"].cpu().numpy()
        got = [float(r["loss_msiv"]), info[0, 0], info[1, 0], info[2, 0], float(r["loss_w"]),
               float(r["loss_c1"]) if r["loss_c1"] is not None else 0.0, float(r["norm"]), float(r["loss_mslv"])]
        ref = g[f"{pre}_losses"]
        for k, (a, b) in enumerate(zip(got, ref)):
            assert abs(a - b) <= (lt if it == 0 else 3 * lt) * abs(b) + 1e-7, (it, k, got, ref.tolist())
        for key in g.files:
            if key.startswith(f"{pre}_grad1:") or key.startswith(f"{pre}_grad2:"):
                phase = 0 if "_grad1:" in key else 1
                k = key.split(":", 1)[1]
                e = l2rel(calls[phase][k], g[key])
                # phase 2 and iteration 1 follow sign-like first Adam steps (see test_embed_gpu.py)
                assert e < (5e-3 if phase == 0 and it == 0 else 6e-2), (it, phase, k, e)
        if opt == "E":
            ck = R.checksum({k: v.cpu() for k, v in E.state_dict().items() if not k.endswith("blur.weight")})
        else:
            ck = R.checksum({"w1": st.w1.detach().cpu()})
        assert abs(ck - float(g[f"{pre}_param_checksum"])) < 2e-4 * float(g[f"{pre}_param_checksum"])


# ------------------------------------------------------------------ p-norm kernel
@pytest.mark.parametrize("shape", [(1, 18, 512), (3, 10, 512)])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_latent_pnorm_kernel_matches_torch(shape, p):
    from dge_amd import ops
    w = R.randn(f"pnorm.{p}.{shape}", shape, 9)
    wd = w.double().requires_grad_(True)
    ref = torch.linalg.vector_norm(wd, ord=p)
    ref.backward()
    wc = w.cuda()
    l2 = torch.empty((), dtype=torch.float32, device=DEV)
    n = ops.latent_pnorm(wc, p, out_l2=l2)
    assert abs(float(n) - float(ref)) <= 1e-6 * float(ref)
    assert abs(float(l2) - float(torch.linalg.vector_norm(w.double()))) <= 1e-6 * float(l2)
    g = torch.ones_like(wc)
    ops.latent_pnorm_bwd(wc, n, g, p, beta=0.5)
    want = 1.0 + 0.5 * wd.grad
    assert ((g.double().cpu() - want).abs().max() / want.abs().max()).item() < 1e-6
    # deterministic: the same bits on a second run
    n2 = ops.latent_pnorm(wc, p)
    g2 = torch.ones_like(wc)
    ops.latent_pnorm_bwd(wc, n2, g2, p, beta=0.5)
    assert torch.equal(n, n2) and torch.equal(g, g2)


@pytest.mark.parametrize("p", [1, 2, 3])
def test_latent_pnorm_zero_input_has_zero_gradient(p):
    from dge_amd import ops
    w = torch.zeros(2, 10, 512, device=DEV)
    n = ops.latent_pnorm(w, p)
    g = torch.zeros_like(w)
    ops.latent_pnorm_bwd(w, n, g, p, beta=1.0)
    assert float(n) == 0.0
    assert torch.isfinite(g).all() and float(g.abs().max()) == 0.0


def test_wplus_lerp_kernel():
    from dge_amd import ops
    w = R.randn("lerp.w", (2, 10, 512), 3).cuda()
    for avg in (R.randn("lerp.avg", (512,), 3).cuda(), R.randn("lerp.avgL", (10, 512), 3).cuda()):
        out = ops.wplus_lerp(w, avg, 0.7)
        ref = avg + 0.7 * (w - avg)
        assert (out - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
    g = R.randn("lerp.g", (2, 10, 512), 4).cuda()
    assert (ops.wplus_lerp_bwd(g, 0.7) - 0.7 * g).abs().max().item() <= 1e-6 * g.abs().max().item()


# ------------------------------------------------------------------ trackers
def host_track(rules, seq, mins):
    """The reference's `if` chains (embedding_v2_styleGAN1.py:128-131, embedding_v2_styleGAN2.py:153-166) in f32 on the host."""
    from dge_amd import ops
    f = np.float32
    ml, mn = f(mins[0]), f(mins[1])
    lh, nh = f(rules["loss_hyst"]), f(rules["norm_hyst"])
    ev = []
    for it, loss, norm in seq:
        loss, norm = f(loss), f(norm)
        if rules["arm_rule"] == ops.TRACK_ARM_AT:
            if it == rules["arm_iter"]:
                ml = loss
            armed = it >= rules["arm_iter"]
        else:
            armed = it > rules["arm_iter"]
        if armed:
            if ml > loss * lh:
                ml = loss
                ev.append((it, 0))
            if nh > 0 and mn > norm * nh:
                mn = norm
                ev.append((it, 1))
    return ev, (float(ml), float(mn))


def _track_run(st, run, n, it0=0):
    seq, ws = [], {}
    for i in range(n):
        r = run()
        torch.cuda.synchronize()
        seq.append((it0 + i, float(r["loss_msiv"]), float(r["w_norm"])))
        ws[it0 + i] = r["w1"].detach().clone()
    return seq, ws


def _check_tracker(st, seq, ws, mins):
    want, mins_after = host_track(st.rules, seq, mins)
    tr = st.tracker()
    assert [(e[0], e[1]) for e in tr["events"]] == want, (tr["events"], want)
    assert tr["iteration"] == seq[-1][0] + 1 and tr["dropped"] == 0
    for kind, key in ((0, "best_loss"), (1, "best_norm")):
        its = [it for it, k in want if k == kind]
        if its:
            assert torch.equal(tr[key], ws[its[-1]]), (kind, its[-1])
    for it, k, loss, norm in tr["events"]:
        assert loss == np.float32(dict((s[0], s[1]) for s in seq)[it])
    assert tr["min_loss"] == mins_after[0] and tr["min_norm"] == mins_after[1]
    return mins_after


@pytest.mark.parametrize("gen", ["sg1", "sg2"])
@pytest.mark.parametrize("launch", ["eager", "graph"])
def test_tracker_matches_host_restatement(gen, launch):
    from dge_amd.embedding_v2 import LatentEmbedStep
    g = golden("embed_v2.npz")
    G, E, LP = make_models(gen)
    st = LatentEmbedStep(G, E, LP, mode="W", generator=gen, lr=0.005, arm_iter=3)
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    tag = f"{gen}_W"
    # every noise tensor on the device: a host tensor would be uploaded inside the captured region
    noises = tuple([n.cuda() for n in l] if l is not None else None for l in case_noises(g, tag, 0))
    begin(st, g, gen, "W", imgs1)
    if launch == "graph":
        st.capture(imgs1, noises, warmup=1)
        begin(st, g, gen, "W", imgs1)              # restart the group: tracker, w1 and Adam state in place, graph intact
        run = st.replay
    else:
        run = lambda: st.step(imgs1, noises)
    seq, ws = _track_run(st, run, 12)
    mins = _check_tracker(st, seq, ws, st.rules["init"])
    if gen == "sg2":
        assert len(st.tracker()["events"]) >= 2              # minima start at 100 / 1000: the first armed iteration improves both
        # second image group: the StyleGAN2 minima carry over, the iteration counter restarts
        img_b = R.randn("embed_v2.second_image", tuple(imgs1.shape), 3, 0.4).cuda().clamp(-1, 1)
        st.begin_image(img_b, w_init=torch.as_tensor(g[f"{tag}_w0"]))
        if launch == "graph":
            st.set_image(img_b)
            run = st.replay
        else:
            run = lambda: st.step(img_b, noises)
        seq, ws = _track_run(st, run, 8)
        _check_tracker(st, seq, ws, mins)


# ------------------------------------------------------------------ frozen encoder
def test_frozen_encoder_backward_computes_the_data_gradient_only(monkeypatch):
    from dge_amd import ops
    from dge_amd.embedding_v2 import LatentEmbedStep
    from dge_amd.autograd_encblur import blur_noises
    g = golden("embed_v2.npz")
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        _, Et, _ = make_models("sg2")
        imgs = torch.as_tensor(g["imgs1"]).cuda()
        ops.noise_seed(5)
        nz = blur_noises(Et, 1, 64, imgs.device)
        gw = R.randn("frozen.gw", (1, 10, 512), 6).cuda()
        gc = R.randn("frozen.gc", (1, 64, 4, 4), 6).cuda()

        def img_grad(E):
            x = imgs.clone().requires_grad_(True)
            c, w = E(x, noises=nz)
            torch.autograd.backward([c, w], [gc, gw])
            return x.grad.clone()
        g_train = img_grad(Et)
        G, Ef, LP = make_models("sg2")
        for p in Ef.parameters():
            p.requires_grad_(False)

        def boom(*a, **kw):
            raise AssertionError("weight-gradient kernel called with a frozen encoder")
        for name in ("conv_wgrad", "conv_wgrad_dots", "fromrgb_bwd", "dense_wgrad"):
            monkeypatch.setattr(ops, name, boom)
        g_frozen = img_grad(Ef)
        assert torch.equal(g_frozen, g_train)
        assert all(p.grad is None for p in Ef.parameters())
        st = LatentEmbedStep(G, Ef, LP, mode="W", generator="sg2", lr=0.005)
        st.begin_image(imgs, w_init=torch.as_tensor(g["sg2_W_w0"]))
        r = st.step(imgs, noises=case_noises(g, "sg2_W", 0))
        torch.cuda.synchronize()
        assert torch.isfinite(r["w1"]).all() and st.w1.grad is not None
        assert all(p.grad is None for p in Ef.parameters())
    finally:
        ops.set_deterministic(was)


# ------------------------------------------------------------------ replay == eager
def test_w_mode_replay_equals_eager_bitwise():
    """W mode, StyleGAN2-64, deterministic mode: 5 replays of the captured iteration give the bits of 5 eager iterations (the eager
    run takes Adam's step factors from the same device scalars, LREQAdam.graph_advance); then a second image group through
    set_image."""
    from dge_amd import ops
    from dge_amd.embedding_v2 import LatentEmbedStep
    g = golden("embed_v2.npz")
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    img_b = R.randn("embed_v2.second_image", tuple(imgs1.shape), 3, 0.4).cuda().clamp(-1, 1)
    w0 = torch.as_tensor(g["sg2_W_w0"])
    noises = case_noises(g, "sg2_W", 0)
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        def eager(img, n):
            G, E, LP = make_models("sg2")
            a = LatentEmbedStep(G, E, LP, mode="W", generator="sg2", lr=0.005)
            a.begin_image(img, w_init=w0)
            a.opt.graph_begin(2, imgs1.device)
            out = []
            for _ in range(n):
                a.opt.graph_advance()
                out.append(a.step(img, noises)["w1"].clone())
            return out
        wa = eager(imgs1, 5)
        G, E, LP = make_models("sg2")
        b = LatentEmbedStep(G, E, LP, mode="W", generator="sg2", lr=0.005)
        b.begin_image(imgs1, w_init=w0)
        b.capture(imgs1, noises, warmup=1)
        b.begin_image(imgs1, w_init=w0)
        wb = [b.replay()["w1"].clone() for _ in range(5)]
        torch.cuda.synchronize()
        for i in range(5):
            assert torch.equal(wa[i], wb[i]), (i, relerr(wb[i], wa[i].cpu().numpy()))
        wa2 = eager(img_b, 2)
        b.begin_image(img_b, w_init=w0)
        b.set_image(img_b)
        wb2 = [b.replay()["w1"].clone() for _ in range(2)]
        torch.cuda.synchronize()
        assert not torch.equal(wb2[0], wb[0])
        for i in range(2):
            assert torch.equal(wa2[i], wb2[i]), i
    finally:
        ops.set_deterministic(was)


# ------------------------------------------------------------------ full size
@pytest.mark.parametrize("opt", ["W", "E"])
def test_fullsize_sg2_1024_bf16_eager_and_replay(opt):
    """StyleGAN2-1024 + E_Blur (9 blocks, 18 W+ rows), bf16, batch 1: 3 eager iterations and 3 replayed ones from the same start
    and the same static noise; all finite, replay within the bf16 band of eager (default atomics mode), and the synthesis runs on
    the generator's default up-layer kernels."""
    from dge_amd import ops
    from dge_amd.embedding_v2 import LatentEmbedStep, build_models_v2
    from dge_amd.autograd_encblur import blur_noises
    from tests.helpers import s2_shapes
    torch.manual_seed(0)
    img = torch.tanh(R.randn("embed_v2.full.img", (1, 3, 1024, 1024), 7, 0.8)).cuda()
    PG = R.fill_s2(s2_shapes(1024), seed=1)

    def make():
        G, E, LP = build_models_v2(2, 1024, 16, "bf16", device=DEV, seed=3)
        G.load_state_dict(PG)
        LP.load_state_dict(LR.seeded_params(0))
        assert G.synthesis.num_layers == 18 and E.layer_count == 9
        return LatentEmbedStep(G, E, LP, mode=opt, generator="sg2", lr=0.005)
    w0 = R.randn("embed_v2.full.w0", (1, 18, 512), 5)
    a = make()
    ops.noise_seed(11)
    noises = (blur_noises(a.E, 1, 1024, img.device), None, blur_noises(a.E, 1, 1024, img.device))
    a.begin_image(img, w_init=w0)
    a.opt.graph_begin(2, img.device)
    log = []
    ops.KERNEL_LOG = log
    try:
        wa = []
        for _ in range(3):
            a.opt.graph_advance()
            r = a.step(img, noises)
            wa.append(r["w1"].clone())
    finally:
        ops.KERNEL_LOG = None
    torch.cuda.synchronize()
    assert any(n.startswith("up_s4") for n, _ in log), sorted({n for n, _ in log})
    assert all(torch.isfinite(w).all() for w in wa) and torch.isfinite(r["imgs2"]).all() and np.isfinite(float(r["loss_msiv"]))
    b = make()
    b.begin_image(img, w_init=w0)
    b.capture(img, noises, warmup=1)
    b.begin_image(img, w_init=w0)
    wb = [b.replay()["w1"].clone() for _ in range(3)]
    torch.cuda.synchronize()
    rb = b.last
    assert all(torch.isfinite(w).all() for w in wb) and np.isfinite(float(rb["loss_msiv"])) and np.isfinite(float(rb["loss_mslv"]))
    # default (atomics) mode in bf16: the first iteration differs by the reduction order alone; beta1 = 0 Adam is sign-like in its
    # first steps, so rounding-level differences of near-zero gradients flip update signs and the spread grows from there (the
    # band of test_embed_gpu.py::test_graph_replay_equals_eager_iterations)
    for i in range(3):
        e = l2rel(wb[i], wa[i].cpu().numpy())
        meas(f"embed_v2.full.{opt}.it{i}", w1_l2=e)
        assert e < (2e-2 if i == 0 else 8e-2), (i, e)
