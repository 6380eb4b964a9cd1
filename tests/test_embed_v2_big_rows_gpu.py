"""The independent-rows form of the BigGAN-deep inversion (dge_amd.embedding_v2_biggan.BigEmbedRowsStep): B = 3 rows with the labels
30 / 207 / 5, mode W without and with the attention terms, against
  * the reference's own loop run at batch 1 per image, every run from the same weight_u / weight_v buffers and the same noise feed
    (tests/golden/embed_v2_big_rows.npz, tools/gen_golden_embed_big_rows.py),
  * a fresh batch-1 BigEmbedStep of the coupled path per row,
and its per-row trackers, its launches and its refusals."""
import functools

import numpy as np
import pytest
import torch

from tests.conftest import MODES, golden, meas
from tests.golden import recipe as R
from tests.test_embed_v2_big_gpu import IMGS2_BOUND, l2rel, make_models, relerr
from tests.test_loss_rows_gpu import _check_info

pytestmark = pytest.mark.gpu
CASES = {"W": False, "W-att": True}
KEY = "embed_v2_big_rows"
B = 3


def _labels(g):
    return [int(v) for v in g["labels"]]


def _noise(g, tag, what, rows):
    """The noise lists of the fixture's batch-1 runs (the same feed for every row), repeated for `rows` rows."""
    shapes = [tuple(s) for s in g[f"{tag}_{'init_noise_shapes' if what == 'init' else 'noise_shapes'}"].tolist()]
    assert all(s[0] == 1 for s in shapes)
    nz = [R.randn(f"{KEY}.{tag}.{what}.noise{i}", s, 2).repeat(rows, *([1] * (len(s) - 1))).cuda() for i, s in enumerate(shapes)]
    if what == "init":
        return nz
    s0, s1 = [int(v) for v in g[f"{tag}_noise_split"].tolist()]
    return (nz[:s0] or None, nz[s0:s1])


def _spy_steps(st, r_step):
    """One step with the w1 gradient of both phases captured (what the optimiser sees)."""
    calls, orig = [], st.opt.step

    def spy(*a, **kw):
        calls.append(st.w1.grad.detach().clone())
        return orig(*a, **kw)
    st.opt.step = spy
    try:
        r = r_step()
    finally:
        st.opt.step = orig
    return r, calls


KEEP = ("w1", "w2", "imgs2", "const1", "const2", "loss_msiv", "loss_imgs", "loss_w", "loss_c2", "loss_mslv", "info_imgs", "mask_2",
        "loss_mask", "loss_Gcam", "info_w", "info_c2")


def _keep(r, calls):
    out = {k: r[k].detach().clone() for k in KEEP if k in r}
    out["grads"] = calls
    return out


@functools.lru_cache(maxsize=None)
def rows_run(tag, det):
    """Two iterations of the B = 3 rows step in the given reduction mode; iteration 0 traced."""
    from dge_amd import ops
    from dge_amd.embedding_v2_biggan import BigEmbedRowsStep
    g = golden(f"{KEY}.npz")
    att = CASES[tag]
    was = ops.is_deterministic()
    ops.set_deterministic(det)
    try:
        G, E, LP, vgg = make_models(att)
        st = BigEmbedRowsStep(G, E, LP, vgg16=vgg, attention=att, lr=0.0003, iterations=2)
        imgs1 = torch.as_tensor(g["imgs1"]).cuda()
        st.begin_image(imgs1, labels=_labels(g), noises=_noise(g, tag, "init", B))
        head = dict(cond_vector=st.cond_vector.clone(), w0=st.w1.detach().clone(), const1=st._const1.clone(),
                    frozen=all(not p.requires_grad for p in E.parameters()), train=G.training and E.training)
        outs, names = [], None
        for it in range(2):
            if it == 0:
                ops.KERNEL_LOG = log = []
            try:
                r, calls = _spy_steps(st, lambda: st.step(imgs1, noises=_noise(g, tag, f"it{it}", B)))
            finally:
                ops.KERNEL_LOG = None
            if it == 0:
                names = [n for n, _ in log]
            outs.append(_keep(r, calls))
        torch.cuda.synchronize()
        return head, outs, names, st.tracker()
    finally:
        ops.set_deterministic(was)


def check_row(name, o, b, ref, it, lt, att):
    """Row b of the rows result `o` against `ref` (arrays of a batch-1 run) with the mode-W bounds of
    tests/test_embed_v2_big_gpu.py::test_big_embed_loop_matches_reference_run (its asserts' literals; IMGS2_BOUND is that module's)."""
    row = lambda k: o[k][b:b + 1]
    got_l = [float(o[k][b]) for k in ("loss_msiv", "loss_imgs", "loss_w", "loss_c2", "loss_mslv")]
    info = o["info_imgs"][b].cpu().numpy()
    e = dict(w1=relerr(row("w1"), ref["w1"]), w1_l2=l2rel(row("w1"), ref["w1"]), w2=relerr(row("w2"), ref["w2"]),
             imgs2=relerr(row("imgs2")[:, :, ::2, ::2], ref["imgs2"]),
             imgs2_norm=abs(float(row("imgs2").norm()) - float(ref["imgs2_norm"])) / float(ref["imgs2_norm"]),
             const2=relerr(row("const2"), ref["const2"]), const1=relerr(row("const1"), ref["const1"]),
             losses=max(abs(a - c) / abs(c) for a, c in zip(got_l, ref["losses"])),
             grad1=l2rel(o["grads"][0][b:b + 1], ref["grad1"]), grad2=l2rel(o["grads"][1][b:b + 1], ref["grad2"]))
    ck = R.checksum({"w1": row("w1").cpu()})
    e["checksum"] = abs(ck - float(ref["checksum"])) / float(ref["checksum"])
    e["info_imgs"] = max(abs(info[1 + c] - ref["info_imgs"][c]) / (abs(ref["info_imgs"][c]) + 1e-6) for c in (0, 4, 5, 6))
    if att:
        e["mask_2"] = float(np.abs(row("mask_2").cpu().numpy() - ref["mask_2"]).max())
        ra = ref["att_losses"]
        e["att_losses"] = max(abs(float(o["loss_mask"][b]) - ra[0]) / abs(ra[0]), abs(float(o["loss_Gcam"][b]) - ra[1]) / abs(ra[1]))
    meas(name, **e)
    assert e["w1_l2"] < 1e-3 and e["w1"] < 4e-3, (b, it, e)
    assert e["w2"] < (2e-3 if it == 0 else 1e-2), (b, it, e)
    assert e["imgs2"] < IMGS2_BOUND["W"][it] and e["imgs2_norm"] < 2e-3, (b, it, e)
    assert e["const2"] < (2e-3 if it == 0 else 1e-2) and e["const1"] < 1e-3, (b, it, e)
    assert e["losses"] <= (lt if it == 0 else 3 * lt), (b, it, got_l, list(ref["losses"]))
    assert e["info_imgs"] < 1e-2, (b, it, e)
    assert e["grad1"] < (5e-3 if it == 0 else 6e-2) and e["grad2"] < 6e-2, (b, it, e)
    assert e["checksum"] < 2e-4, (b, it, e)
    if att:
        assert e["mask_2"] < 5e-3 and e["att_losses"] < 5e-3, (b, it, e)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag", list(CASES))
def test_big_embed_rows_match_reference_run_per_image(tag, mode):
    g = golden(f"{KEY}.npz")
    att = CASES[tag]
    head, outs, names, tr = rows_run(tag, mode == "det")
    assert head["train"] and head["frozen"]
    lt = 1e-3 if mode == "det" else 3e-3
    for b in range(B):
        assert relerr(head["cond_vector"][b:b + 1], g[f"{tag}_cond_vector"][b:b + 1]) < 1e-5
        assert relerr(head["w0"][b:b + 1], g[f"{tag}_w0"][b:b + 1]) < 1e-3
        assert relerr(head["const1"][b:b + 1], g[f"{tag}_const1"][b:b + 1]) < 1e-3
        for it in range(2):
            pre = f"{tag}_it{it}"
            ref = dict(w1=g[f"{pre}_w1"][b:b + 1], w2=g[f"{pre}_w2"][b:b + 1], imgs2=g[f"{pre}_imgs2"][b:b + 1],
                       imgs2_norm=g[f"{pre}_imgs2_norm"][b], const2=g[f"{pre}_const2"][b:b + 1], const1=g[f"{tag}_const1"][b:b + 1],
                       losses=g[f"{pre}_losses"][b], grad1=g[f"{pre}_grad1:w1"][b:b + 1], grad2=g[f"{pre}_grad2:w1"][b:b + 1],
                       checksum=g[f"{pre}_param_checksum"][b], info_imgs=g[f"{pre}_info"][b, 0])
            if att:
                ref.update(mask_2=g[f"{pre}_mask_2"][b:b + 1], att_losses=g[f"{pre}_att_losses"][b])
            check_row(f"embed_v2_big_rows.{tag}.{mode}.row{b}.it{it}", outs[it], b, ref, it, lt, att)
    assert [t["iteration"] for t in tr] == [2] * B and all(t["dropped"] == 0 for t in tr)


@pytest.mark.parametrize("tag", list(CASES))
def test_big_embed_rows_equal_batch_one_runs_of_the_coupled_step(tag):
    """Every row against a fresh batch-1 BigEmbedStep with that row's label, started from the same (freshly loaded) weight_u /
    weight_v buffers, in deterministic mode; and the coupled B = 3 step is another computation."""
    from dge_amd import ops
    from dge_amd.embedding_v2_biggan import BigEmbedStep
    g = golden(f"{KEY}.npz")
    att = CASES[tag]
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        head, outs, names, _ = rows_run(tag, True)
        imgs = torch.as_tensor(g["imgs1"]).cuda()
        lt = 1e-3
        for b in range(B):
            G, E, LP, vgg = make_models(att)
            st = BigEmbedStep(G, E, LP, mode="W", vgg16=vgg, attention=att, label=_labels(g)[b], lr=0.0003, iterations=2)
            st.begin_image(imgs[b:b + 1], noises=_noise(g, tag, "init", 1))
            assert relerr(head["cond_vector"][b:b + 1], st.cond_vector.cpu().numpy()) < 1e-6
            for it in range(2):
                r, calls = _spy_steps(st, lambda: st.step(imgs[b:b + 1], noises=_noise(g, tag, f"it{it}", 1)))
                n = lambda k: r[k].detach().cpu().numpy()
                ref = dict(w1=n("w1"), w2=n("w2"), imgs2=n("imgs2")[:, :, ::2, ::2], imgs2_norm=float(r["imgs2"].norm()), const2=n("const2"),
                           const1=n("const1"), losses=[float(r[k]) for k in ("loss_msiv", "loss_imgs", "loss_w", "loss_c2", "loss_mslv")],
                           grad1=calls[0].cpu().numpy(), grad2=calls[1].cpu().numpy(), checksum=R.checksum({"w1": r["w1"].cpu()}),
                           info_imgs=n("info_imgs")[1:])
                if att:
                    ref.update(mask_2=n("mask_2"), att_losses=[float(r["loss_mask"]), float(r["loss_Gcam"])])
                check_row(f"embed_v2_big_rows.single.{tag}.row{b}.it{it}", outs[it], b, ref, it, lt, att)
                # the logged terms of the two latent losses (the KL of the 2-D w is the softmax over the row's features, as in the
                # one-row space_loss): the bound tests/test_loss_rows_gpu.py applies to a rows form's logged terms
                for key in ("info_w", "info_c2"):
                    _check_info(outs[it][key][b].cpu(), r[key].cpu(), (key, b, it))
                assert float(r["info_w"][4]) > 0.0
        # the coupled B = 3 step (one label, one loss for the batch) is a different computation: its loss_msiv is not row 0's
        G, E, LP, vgg = make_models(att)
        st = BigEmbedStep(G, E, LP, mode="W", vgg16=vgg, attention=att, label=_labels(g)[0], lr=0.0003, iterations=2)
        st.begin_image(imgs, noises=_noise(g, tag, "init", B))
        c = float(st.step(imgs, noises=_noise(g, tag, "it0", B))["loss_msiv"])
        mine = float(outs[0]["loss_msiv"][0])
        meas(f"embed_v2_big_rows.coupled.{tag}", coupled=c, row0=mine)
        assert abs(c - mine) > 10 * lt * abs(mine), (c, mine)
    finally:
        ops.set_deterministic(was)


COUPLED_ENTRIES = ("dge_class_target", "dge_gather_row", "dge_mask2cam", "dge_embed_track", "dge_latent_pnorm_fwd", "dge_loss_reduce",
                   "dge_loss_reduce3", "dge_space_loss_finalize", "dge_space_loss_bwd")


def test_big_embed_rows_step_launches_only_the_per_row_forms(monkeypatch):
    """The traced step names the per-row launches and none of the coupled ones; and a step runs with every batch-coupled entry point
    (the class target, the broadcast gather, mask2cam's recurrence, the single tracker, the batch reductions) made unreachable."""
    from dge_amd._lib import lib
    from dge_amd.embedding_v2_biggan import BigEmbedRowsStep
    _, _, names, _ = rows_run("W-att", True)
    for coupled in ("class_target", "mask2cam", "embed_track"):
        assert coupled not in names, coupled
    assert names.count("class_target_rows") == 2 and names.count("gather_rows") == 2 and names.count("mask2cam_rows") == 2
    assert names.count("embed_track_rows") == 1 and "space_loss_finalize_rows" in names
    _, _, plain, _ = rows_run("W", True)
    assert "class_target_rows" not in plain and plain.count("embed_track_rows") == 1
    g = golden(f"{KEY}.npz")
    G, E, LP, vgg = make_models(True)
    st = BigEmbedRowsStep(G, E, LP, vgg16=vgg, attention=True, lr=0.0003, iterations=2)
    imgs = torch.as_tensor(g["imgs1"]).cuda()
    st.begin_image(imgs, labels=_labels(g))

    def boom(*a, **kw):
        raise AssertionError("batch-coupled entry point called by a rows step")
    for name in COUPLED_ENTRIES:
        monkeypatch.setattr(lib(), name, boom)
    r = st.step(imgs)
    assert tuple(r["loss_msiv"].shape) == (B,) and torch.isfinite(r["loss_msiv"]).all()


def test_big_embed_rows_trackers_follow_the_host_rule_per_row():
    """A tracker per row (tracker_rules("sg1", iterations), armed at arm_iter): events, minima and best latents of every row against
    the host restatement on that row's own loss sequence; a new group restarts every row."""
    from dge_amd.embedding_v2_biggan import BigEmbedRowsStep
    from tests.test_embed_v2_gpu import host_track
    g = golden(f"{KEY}.npz")
    G, E, LP, _ = make_models(False)
    st = BigEmbedRowsStep(G, E, LP, attention=False, lr=0.0003, iterations=2, arm_iter=2)
    imgs = torch.as_tensor(g["imgs1"]).cuda()
    st.begin_image(imgs, labels=_labels(g), noises=_noise(g, "W", "init", B))
    noises = _noise(g, "W", "it0", B)
    seqs, ws = [[] for _ in range(B)], [{} for _ in range(B)]
    for i in range(6):
        r = st.step(imgs, noises)
        lm, wn = r["loss_msiv"].cpu(), r["w_norm"].cpu()
        for b in range(B):
            seqs[b].append((i, float(lm[b]), float(wn[b])))
            ws[b][i] = r["w1"][b:b + 1].clone()
    tr = st.tracker()
    assert isinstance(tr, list) and len(tr) == B
    for b in range(B):
        want, mins = host_track(st.rules, seqs[b], st.rules["init"])
        assert [(ev[0], ev[1]) for ev in tr[b]["events"]] == want and tr[b]["iteration"] == 6 and tr[b]["dropped"] == 0, (b, tr[b]["events"], want)
        assert tr[b]["min_loss"] == mins[0]
        if want:
            assert torch.equal(tr[b]["best_loss"], ws[b][want[-1][0]])
    assert len({tuple(t["events"]) for t in tr}) > 1 or len({t["min_loss"] for t in tr}) == B          # the rows are tracked apart
    st.begin_image(imgs, labels=[5, 5, 5])          # a new group with other labels: conditions rebuilt, every row restarts
    assert st.labels == (5, 5, 5) and torch.equal(st.conditions.argmax(1).cpu(), torch.tensor([5, 5, 5]))
    assert torch.equal(st.cond_vector[0], st.cond_vector[1])
    for t in st.tracker():
        assert t["iteration"] == 0 and t["events"] == [] and t["min_loss"] == 0.0


def test_big_embed_rows_refusals():
    from dge_amd import embedding_v2_biggan as M
    g = golden(f"{KEY}.npz")
    G, E, LP, _ = make_models(False)
    with pytest.raises(ValueError, match="mode 'W' only"):
        M.BigEmbedRowsStep(G, E, LP, mode="E", attention=False)
    with pytest.raises(ValueError, match="independent=True is not offered.*BigEmbedRowsStep"):
        M.BigEmbedStep(G, E, LP, mode="W", attention=False, independent=True)
    st = M.BigEmbedRowsStep(G, E, LP, attention=False, iterations=2)
    imgs = torch.as_tensor(g["imgs1"]).cuda()
    with pytest.raises(ValueError, match="hipGraph capture / replay is not offered"):
        st.capture(imgs)
    with pytest.raises(ValueError, match="hipGraph capture / replay is not offered"):
        st.replay()
    with pytest.raises(ValueError):
        st.begin_image(imgs, labels=[30, 207])
    with pytest.raises(ValueError):
        st.begin_image(imgs, labels=[30, 207, 1000])
    st.begin_image(imgs)          # default: the constructor's label for every row
    assert st.labels == (30, 30, 30)
