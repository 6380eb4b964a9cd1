"""LatentEmbedStep(independent=True) (dge_amd.embedding_v2): the rows of a W-mode batch as inversions of their own.  Row 0 of a
B = 3 batch against the reference's own batch-1 run (tests/golden/embed_v2.npz), every row against a fresh batch-1 step of the
coupled path on that row's inputs, the per-row trackers against the host restatement of the reference's `if` chains, graph
replay, the launch log, and StyleGAN2-1024 in bf16 at B = 2."""
import functools

import numpy as np
import pytest
import torch

from tests.conftest import MODES, golden, meas
from tests.golden import recipe as R
from oracle import lpips_ref as LR
from tests.test_embed_v2_gpu import host_track, l2rel, make_models, relerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3
ROW_KERNELS = {"loss_reduce_rows", "loss_reduce_rows_c3v4", "ssim_fwd_rows", "space_loss_finalize_rows", "space_loss_bwd_rows",
               "space_loss_bwd_rows_v4", "latent_pnorm_rows_fwd", "latent_pnorm_rows_bwd", "embed_track_rows"}
# the entry points whose sums run over the whole batch (and the single tracker): an independent step must not reach them
COUPLED_ENTRIES = ["dge_loss_reduce", "dge_loss_reduce3", "dge_ssim_fwd", "dge_space_loss_finalize", "dge_space_loss_bwd",
                   "dge_space_loss_bwd3", "dge_space_loss_bwd_split", "dge_latent_pnorm_fwd", "dge_latent_pnorm_bwd", "dge_embed_track"]


@functools.lru_cache(maxsize=None)
def models(gen):
    """Shared by the tests of this module: W mode leaves generator, encoder and LPIPS as they are."""
    return make_models(gen)


def batch_inputs(gen):
    """imgs [B,3,64,64], W+ start codes (StyleGAN2) or init noises (StyleGAN1), and noises(it): row 0 is the golden case, rows 1-2
    are other seeded images in [-1, 1], codes and noises."""
    g = golden("embed_v2.npz")
    tag = f"{gen}_W"
    imgs = torch.cat([torch.as_tensor(g["imgs1"])] +
                     [R.randn(f"embed_rows.img{r}", (1, 3, 64, 64), 3, 0.3 * r).clamp(-1, 1) for r in range(1, B)]).cuda()
    if gen == "sg1":
        shapes = [tuple(s) for s in g[f"{tag}_init_noise_shapes"].tolist()]
        init = dict(noises=[torch.cat([R.randn(f"embed_v2.{tag}.init.noise{i}", s, 2)] +
                                      [R.randn(f"embed_rows.{tag}.r{r}.init.noise{i}", s, 2) for r in range(1, B)]).cuda()
                            for i, s in enumerate(shapes)])
    else:
        init = dict(w_init=torch.cat([torch.as_tensor(g[f"{tag}_w0"])] + [R.randn(f"embed_rows.w0.{r}", (1, 10, 512), 5) for r in range(1, B)]))
    shapes = [tuple(s) for s in g[f"{tag}_noise_shapes"].tolist()]
    s0, s1, s2 = [int(v) for v in g[f"{tag}_noise_split"].tolist()]

    def noises(it):
        nz = [torch.cat([R.randn(f"embed_v2.{tag}.it{it}.noise{i}", s, 2)] +
                        [R.randn(f"embed_rows.{tag}.r{r}.it{it}.noise{i}", s, 2) for r in range(1, B)]) for i, s in enumerate(shapes)]
        return ([n.cuda() for n in nz[:s0]] or None, [n.cuda() for n in nz[s0:s1]] or None, [n.cuda() for n in nz[s1:s2]])
    return g, imgs, init, noises


def row_of(x, r):
    """Row r of a batch input: tensors, lists of tensors and dicts of them"""
    if x is None:
        return None
    if torch.is_tensor(x):
        return x[r:r + 1].contiguous()
    if isinstance(x, dict):
        return {k: row_of(v, r) for k, v in x.items()}
    return type(x)(row_of(v, r) for v in x)


def run_two_iterations(st, imgs, noises):
    """Two iterations with the gradient both optimizer calls see; everything cloned."""
    out = []
    for it in range(2):
        calls = []
        orig = st.opt.step

        def spy(*a, **kw):
            calls.append(st.w1.grad.detach().clone())
            return orig(*a, **kw)
        st.opt.step = spy
        try:
            r = st.step(imgs, noises=noises(it))
        finally:
            st.opt.step = orig
        torch.cuda.synchronize()
        rec = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in r.items()}
        rec["grads"] = calls
        out.append(rec)
    return out


@functools.lru_cache(maxsize=None)
def independent_run(gen, det):
    """The B = 3 independent run of two iterations in the reduction mode that is switched on (`det`: the cache key)."""
    from dge_amd import ops
    from dge_amd.embedding_v2 import LatentEmbedStep
    assert ops.is_deterministic() == det
    g, imgs, init, noises = batch_inputs(gen)
    G, E, LP = models(gen)
    st = LatentEmbedStep(G, E, LP, mode="W", generator=gen, lr=0.005, independent=True)
    st.begin_image(imgs, **init)
    return run_two_iterations(st, imgs, noises)


def eight_losses(r, row=None):
    """The loss numbers of the golden `_losses` entry; `row`: of that row of an independent result"""
    pick = (lambda t: float(t)) if row is None else (lambda t: float(t[row]))
    info = (r["info_img"] if row is None else r["info_img"][row]).cpu().numpy()
    return [pick(r["loss_msiv"]), info[0, 0], info[1, 0], info[2, 0], pick(r["loss_w"]),
            pick(r["loss_c1"]) if r["loss_c1"] is not None else 0.0, pick(r["norm"]), pick(r["loss_mslv"])]


def check_row(name, got, row, ref, it, lt):
    """The bounds test_embed_v2_loop_matches_reference_run applies to its W cases, on row `row` of the independent result `got`;
    `ref`: dict with w1, w2, imgs2, const3, const2 (or None), losses [8], grads [2] (or None), checksum (or None)."""
    e_w1 = relerr(got["w1"][row:row + 1], ref["w1"])
    m = dict(w1=e_w1, w1_l2=l2rel(got["w1"][row:row + 1], ref["w1"]), w2=relerr(got["w2"][row:row + 1], ref["w2"]))
    assert m["w1_l2"] < 1e-3 and e_w1 < 4e-3, (it, m)
    assert m["w2"] < (2e-3 if it == 0 else 1e-2), (it, m)
    if ref.get("imgs2") is not None:
        m["imgs2"] = relerr(got["imgs2"][row:row + 1], ref["imgs2"])
        assert m["imgs2"] < 2e-3, (it, m)
    m["const3"] = relerr(got["const3"][row:row + 1], ref["const3"])
    assert m["const3"] < (2e-3 if it == 0 else 1e-2), (it, m)
    if ref.get("const2") is not None:
        assert relerr(got["const2"][row:row + 1], ref["const2"]) < 1e-3
    else:
        assert got["const2"] is None and got["loss_c1"] is None
    have = eight_losses(got, row)
    for k, (a, b) in enumerate(zip(have, ref["losses"])):
        m[f"loss{k}"] = abs(a - b) / (abs(b) + 1e-30)
        assert abs(a - b) <= (lt if it == 0 else 3 * lt) * abs(b) + 1e-7, (it, k, have, list(ref["losses"]))
    for phase in range(2):
        if ref["grads"][phase] is not None:
            e = l2rel(got["grads"][phase][row:row + 1], ref["grads"][phase])
            m[f"grad{phase + 1}"] = e
            assert e < (5e-3 if phase == 0 and it == 0 else 6e-2), (it, phase, e)
    ck = R.checksum({"w1": got["w1"][row:row + 1].cpu()})
    want = ref["checksum"] if ref.get("checksum") is not None else R.checksum({"w1": torch.as_tensor(np.asarray(ref["w1"])).float()})
    assert abs(ck - want) < 2e-4 * want
    meas(name, **m)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gen", ["sg1", "sg2"])
def test_independent_row0_matches_reference_run(gen, mode):
    from dge_amd import ops
    g = golden("embed_v2.npz")
    tag = f"{gen}_W"
    out = independent_run(gen, ops.is_deterministic())
    lt = 1e-3 if mode == "det" else 3e-3
    for it in range(2):
        pre = f"{tag}_it{it}"
        opt = lambda k: g[f"{pre}_{k}"] if f"{pre}_{k}" in g.files else None
        ref = dict(w1=g[f"{pre}_w1"], w2=g[f"{pre}_w2"], imgs2=opt("imgs2"), const3=g[f"{pre}_const3"], const2=opt("const2"),
                   losses=g[f"{pre}_losses"], grads=[opt("grad1:w1"), opt("grad2:w1")], checksum=float(g[f"{pre}_param_checksum"]))
        check_row(f"embed_rows.row0.{tag}.{mode}.it{it}", out[it], 0, ref, it, lt)


@pytest.mark.parametrize("gen", ["sg1", "sg2"])
def test_independent_rows_equal_single_row_runs(gen):
    """Every row of the B = 3 independent run against a fresh batch-1 step of the coupled path on that row's inputs (deterministic
    mode).  The bounds are what one HIP run may differ from the reference's run: two HIP runs of the same arithmetic are inside."""
    from dge_amd import ops
    from dge_amd.embedding_v2 import LatentEmbedStep
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        out = independent_run(gen, True)
        g, imgs, init, noises = batch_inputs(gen)
        G, E, LP = models(gen)
        lt = 1e-3
        for r in range(B):
            st = LatentEmbedStep(G, E, LP, mode="W", generator=gen, lr=0.005)
            st.begin_image(row_of(imgs, r), **row_of(init, r))
            one = run_two_iterations(st, row_of(imgs, r), lambda it: row_of(noises(it), r))
            for it in range(2):
                o = one[it]
                ref = dict(w1=o["w1"].cpu().numpy(), w2=o["w2"].cpu().numpy(), imgs2=o["imgs2"].cpu().numpy(), const3=o["const3"].cpu().numpy(),
                           const2=o["const2"].cpu().numpy() if o["const2"] is not None else None, losses=eight_losses(o),
                           grads=[x.cpu().numpy() for x in o["grads"]])
                check_row(f"embed_rows.row{r}.{gen}.it{it}", out[it], r, ref, it, lt)
        # the coupled B = 3 step is a different computation: its loss_msiv (one number for the batch) is not row 0's
        st = LatentEmbedStep(G, E, LP, mode="W", generator=gen, lr=0.005)
        st.begin_image(imgs, **init)
        c = float(st.step(imgs, noises=noises(0))["loss_msiv"])
        mine = float(out[0]["loss_msiv"][0])
        meas(f"embed_rows.coupled.{gen}", coupled=c, row0=mine)
        assert abs(c - mine) > 10 * lt * abs(mine), (c, mine)
    finally:
        ops.set_deterministic(was)


def test_independent_needs_w_mode():
    from dge_amd.embedding_v2 import LatentEmbedStep
    G, E, LP = models("sg2")
    with pytest.raises(ValueError):
        LatentEmbedStep(G, E, LP, mode="E", generator="sg2", independent=True)


# ------------------------------------------------------------------ trackers
def _check_row_tracker(st, tr, seq, ws, mins, row):
    want, mins_after = host_track(st.rules, seq, mins)
    assert [(e[0], e[1]) for e in tr["events"]] == want, (row, tr["events"], want)
    assert tr["iteration"] == seq[-1][0] + 1 and tr["dropped"] == 0
    for kind, key in ((0, "best_loss"), (1, "best_norm")):
        its = [it for it, k in want if k == kind]
        if its:
            assert torch.equal(tr[key], ws[its[-1]]), (row, kind, its[-1])
    by_it = dict((s[0], s) for s in seq)
    for it, k, loss, norm in tr["events"]:
        assert loss == np.float32(by_it[it][1]) and norm == np.float32(by_it[it][2])
    assert tr["min_loss"] == mins_after[0] and tr["min_norm"] == mins_after[1]


def _track_rows(st, run, n):
    seqs, ws = [[] for _ in range(B)], [{} for _ in range(B)]
    for i in range(n):
        r = run()
        torch.cuda.synchronize()
        lm, wn = r["loss_msiv"].cpu(), r["w_norm"].cpu()
        for b in range(B):
            seqs[b].append((i, float(lm[b]), float(wn[b])))
            ws[b][i] = r["w1"][b:b + 1].detach().clone()
    return seqs, ws


@pytest.mark.parametrize("gen", ["sg1", "sg2"])
@pytest.mark.parametrize("launch", ["eager", "graph"])
def test_row_trackers_match_host_restatement(gen, launch):
    """A tracker per row: events, minima and best latents of every row against the host restatement run on that row's own loss and
    norm sequence; a second group restarts the minima of every row (both generators)."""
    from dge_amd.embedding_v2 import LatentEmbedStep
    g, imgs, init, noises_of = batch_inputs(gen)
    G, E, LP = models(gen)
    st = LatentEmbedStep(G, E, LP, mode="W", generator=gen, lr=0.005, arm_iter=3, independent=True)
    noises = tuple([n.cuda() for n in l] if l is not None else None for l in noises_of(0))
    if gen == "sg2":
        # row 2 inverts the image of its own start code: its loss starts near its minimum while rows 0 - 1 still fall
        with torch.no_grad():
            st.begin_image(imgs, **init)
            imgs = imgs.clone()
            imgs[2:3] = st._generate(st.w1.detach()[2:3], None)
    st.begin_image(imgs, **init)
    if launch == "graph":
        st.capture(imgs, noises, warmup=1)
        st.begin_image(imgs, **init)
        run = st.replay
    else:
        run = lambda: st.step(imgs, noises)
    seqs, ws = _track_rows(st, run, 12)
    trs = st.tracker()
    assert isinstance(trs, list) and len(trs) == B
    for b in range(B):
        _check_row_tracker(st, trs[b], seqs[b], ws[b], st.rules["init"], b)
    events = [tuple((e[0], e[1]) for e in tr["events"]) for tr in trs]
    print("MEAS row_tracker_events", gen, launch, events)
    assert all(len(e) >= 1 for e in events) and len(set(events)) > 1          # the rows cross their minima at different iterations
    assert len({tuple(e[2] for e in tr["events"]) for tr in trs}) == B          # every row logged its own losses
    # second group (rows in another order): counters, events and the minima of every row restart
    imgs_b = imgs.flip(0).contiguous()
    st.begin_image(imgs_b, **init)
    if launch == "graph":
        st.set_image(imgs_b)
        run = st.replay
    else:
        run = lambda: st.step(imgs_b, noises)
    seqs, ws = _track_rows(st, run, 6)
    for b, tr in enumerate(st.tracker()):
        _check_row_tracker(st, tr, seqs[b], ws[b], st.rules["init"], b)


# ------------------------------------------------------------------ replay == eager
def test_independent_replay_equals_eager_bitwise():
    """StyleGAN2-64, B = 3, deterministic mode: replays of the captured independent iteration give the bits of the eager
    iterations; then a second image group through set_image + begin_image on the same graph."""
    from dge_amd import ops
    from dge_amd.embedding_v2 import LatentEmbedStep
    g, imgs, init, noises_of = batch_inputs("sg2")
    noises = noises_of(0)
    imgs_b = imgs.flip(0).contiguous()
    G, E, LP = models("sg2")
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        def eager(img, n):
            a = LatentEmbedStep(G, E, LP, mode="W", generator="sg2", lr=0.005, independent=True)
            a.begin_image(img, **init)
            a.opt.graph_begin(2, img.device)
            out = []
            for _ in range(n):
                a.opt.graph_advance()
                r = a.step(img, noises)
                out.append((r["w1"].clone(), r["loss_msiv"].clone()))
            return out
        wa = eager(imgs, 3)
        b = LatentEmbedStep(G, E, LP, mode="W", generator="sg2", lr=0.005, independent=True)
        b.begin_image(imgs, **init)
        b.capture(imgs, noises, warmup=1)
        b.begin_image(imgs, **init)
        wb = []
        for _ in range(3):
            r = b.replay()
            wb.append((r["w1"].clone(), r["loss_msiv"].clone()))
        torch.cuda.synchronize()
        for i in range(3):
            assert torch.equal(wa[i][0], wb[i][0]) and torch.equal(wa[i][1], wb[i][1]), i
        wa2 = eager(imgs_b, 2)
        b.begin_image(imgs_b, **init)
        b.set_image(imgs_b)
        wb2 = [b.replay()["w1"].clone() for _ in range(2)]
        torch.cuda.synchronize()
        assert not torch.equal(wb2[0], wb[0][0])
        for i in range(2):
            assert torch.equal(wa2[i][0], wb2[i]), i
    finally:
        ops.set_deterministic(was)


# ------------------------------------------------------------------ several captured steps in one process
def test_tables_a_captured_graph_reads_outlive_a_call_at_another_batch_size():
    """A captured iteration holds the addresses of the generator's style index tables, of the encoder's head table and of the
    noise seed scalar.  A step at another batch size on the same models (tools/bench_embed_v2.py keeps one captured step per
    batch size) must find them kept, not replaced: replaying the first graph would otherwise index through freed memory."""
    from dge_amd import ops
    from dge_amd.autograd_enc import heads_layout
    from dge_amd.autograd_s2 import _style_tables
    from dge_amd.stylegan2_generator import _dt
    G, E, LP = models("sg2")
    dev = torch.device("cuda", torch.cuda.current_device())
    dt = _dt(G.synthesis.compute_dtype)
    t1, h1 = _style_tables(G.synthesis, 1, dt), heads_layout(E, 1, dev)
    t3, h3 = _style_tables(G.synthesis, 3, dt), heads_layout(E, 3, dev)
    assert t3 is not t1 and h3 is not h1 and t3["ybase"].data_ptr() != t1["ybase"].data_ptr()
    assert _style_tables(G.synthesis, 1, dt) is t1 and heads_layout(E, 1, dev) is h1
    assert _style_tables(G.synthesis, 3, dt) is t3 and heads_layout(E, 3, dev) is h3
    ops.noise_graph_begin(dev)
    seed = ops.NOISE.seed_dev
    ops.noise_graph_begin("cuda")
    assert ops.NOISE.seed_dev is seed


def test_two_captured_steps_of_different_batch_sizes_replay_in_turn():
    """StyleGAN2-64, deterministic mode: a coupled batch-1 step and an independent B = 3 step captured on the same models and
    replayed in turn give the bits of each one replayed alone."""
    from dge_amd import ops
    from dge_amd.embedding_v2 import LatentEmbedStep
    g, imgs, init, noises_of = batch_inputs("sg2")
    noises = noises_of(0)
    G, E, LP = models("sg2")
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        def captured(rows):
            st = LatentEmbedStep(G, E, LP, mode="W", generator="sg2", lr=0.005, independent=rows > 1)
            x, w0, nz = (imgs, init, noises) if rows > 1 else (row_of(imgs, 0), row_of(init, 0), row_of(noises, 0))
            st.begin_image(x, **w0)
            st.capture(x, nz, warmup=1)
            st.begin_image(x, **w0)
            return st
        alone = {}
        for rows in (1, B):
            st = captured(rows)
            alone[rows] = [st.replay()["w1"].clone() for _ in range(3)]
            del st
        torch.cuda.synchronize()
        a, b = captured(1), captured(B)
        for i in range(3):
            wa, wb = a.replay()["w1"].clone(), b.replay()["w1"].clone()
            torch.cuda.synchronize()
            assert torch.equal(wa, alone[1][i]) and torch.equal(wb, alone[B][i]), i
    finally:
        ops.set_deterministic(was)


# ------------------------------------------------------------------ launches
@pytest.mark.parametrize("gen", ["sg1", "sg2"])
def test_independent_step_launches(gen, monkeypatch):
    """An independent step reaches none of the batch-coupled reduction entry points and logs the per-sample kernels; the coupled
    step logs none of them, and apart from them the two steps launch the same kernels in the same order."""
    from dge_amd import ops
    from dge_amd._lib import lib
    from dge_amd.embedding_v2 import LatentEmbedStep
    g, imgs, init, noises_of = batch_inputs(gen)
    G, E, LP = models(gen)

    def logged(independent):
        st = LatentEmbedStep(G, E, LP, mode="W", generator=gen, lr=0.005, independent=independent)
        st.begin_image(imgs, **init)
        log = []
        ops.KERNEL_LOG = log
        try:
            st.step(imgs, noises_of(0))
        finally:
            ops.KERNEL_LOG = None
        torch.cuda.synchronize()
        return [n for n, _ in log]
    coupled = logged(False)
    assert not ROW_KERNELS & set(coupled), sorted(ROW_KERNELS & set(coupled))

    def boom(*a, **kw):
        raise AssertionError("batch-coupled entry point called by an independent step")
    for name in COUPLED_ENTRIES:
        monkeypatch.setattr(lib(), name, boom)
    ind = logged(True)
    want = {"loss_reduce_rows", "ssim_fwd_rows", "space_loss_finalize_rows", "space_loss_bwd_rows_v4", "latent_pnorm_rows_fwd",
            "latent_pnorm_rows_bwd", "embed_track_rows"}
    assert want <= set(ind), sorted(want - set(ind))
    assert [n for n in ind if n not in ROW_KERNELS] == coupled


# ------------------------------------------------------------------ full size
def test_fullsize_sg2_1024_bf16_independent_eager_and_replay():
    """StyleGAN2-1024 + E_Blur, bf16, B = 2 independent rows: 3 eager iterations and 3 replayed ones from the same start; all finite,
    replay within the band test_fullsize_sg2_1024_bf16_eager_and_replay allows between the two in the default (atomics) mode."""
    from dge_amd import ops
    from dge_amd.embedding_v2 import LatentEmbedStep, build_models_v2
    from dge_amd.autograd_encblur import blur_noises
    from tests.helpers import s2_shapes
    torch.manual_seed(0)
    img = torch.tanh(R.randn("embed_rows.full.img", (2, 3, 1024, 1024), 7, 0.8)).cuda()
    PG = R.fill_s2(s2_shapes(1024), seed=1)

    def make():
        G, E, LP = build_models_v2(2, 1024, 16, "bf16", device=DEV, seed=3)
        G.load_state_dict(PG)
        LP.load_state_dict(LR.seeded_params(0))
        return LatentEmbedStep(G, E, LP, mode="W", generator="sg2", lr=0.005, independent=True)
    w0 = R.randn("embed_rows.full.w0", (2, 18, 512), 5)
    a = make()
    ops.noise_seed(11)
    noises = (None, None, blur_noises(a.E, 2, 1024, img.device))
    a.begin_image(img, w_init=w0)
    a.opt.graph_begin(2, img.device)
    wa = []
    for _ in range(3):
        a.opt.graph_advance()
        r = a.step(img, noises)
        wa.append(r["w1"].clone())
    torch.cuda.synchronize()
    assert all(torch.isfinite(w).all() for w in wa) and torch.isfinite(r["imgs2"]).all()
    assert tuple(r["loss_msiv"].shape) == (2,) and torch.isfinite(r["loss_msiv"]).all() and torch.isfinite(r["loss_mslv"]).all()
    del a
    b = make()
    b.begin_image(img, w_init=w0)
    b.capture(img, noises, warmup=1)
    b.begin_image(img, w_init=w0)
    wb = [b.replay()["w1"].clone() for _ in range(3)]
    torch.cuda.synchronize()
    rb = b.last
    assert all(torch.isfinite(w).all() for w in wb) and torch.isfinite(rb["loss_msiv"]).all() and torch.isfinite(rb["loss_mslv"]).all()
    for i in range(3):
        e = l2rel(wb[i], wa[i].cpu().numpy())
        meas(f"embed_rows.full.it{i}", w1_l2=e)
        assert e < (2e-2 if i == 0 else 8e-2), (i, e)
