"""Noise optimisation in the v2 inversion loop (dge_amd.embedding_v2.LatentEmbedStep(optimize_noise=True): StyleGAN2, mode "W"):
two iterations against the loop composed from the reference's generator (its noise buffers as leaves), E_Blur, space_loss and
LREQAdam (tests/golden/embed_v2_noise.npz, tools/gen_golden_s2_noise.py) inside the mode-W bounds of tests/test_embed_v2_gpu.py;
independent rows against their batch-1 runs (the bounds of tests/test_embed_rows_gpu.py); what phase 2 and the switched-off flag
leave alone; the files of a group; graph replay against eager."""
import os

import pytest
import torch

from tests.conftest import MODES, golden, meas
from tests.golden import recipe as R
from tests.s2_noise_models import S2N_RES, s2n_state_dict
from tests.test_embed_v2_gpu import l2rel, make_models, relerr

pytestmark = pytest.mark.gpu
L = 5
# relative L2 of the maps and of their phase-1 gradients against the reference loop: 3x the largest value measured on the MI355X
# over both iterations and both modes (README, "Noise optimisation"), the project's rule for a quantity without an earlier bound.
# L2 because beta_1 = 0 makes an element's first Adam step lr * sign(g): an element whose gradient is within rounding of zero may
# step the other way.  No element is excluded.
NOISE_L2_BOUND = 3 * 2.61e-8
NOISE_GRAD_L2_BOUND = 3 * 1.84e-7


def make_step(**kw):
    from dge_amd.embedding_v2 import LatentEmbedStep
    G, E, LP = make_models("sg2")
    G.load_state_dict(s2n_state_dict())
    return LatentEmbedStep(G, E, LP, mode="W", generator="sg2", lr=0.005, **kw)


def enc_noises(g, it, name="embed_v2_noise", rows=slice(None), nb=None):
    """(unused, unused, E(imgs2)) noise lists of iteration `it` (the synthesis noise is the maps)."""
    shapes = [tuple(s) for s in g["noise_shapes"].tolist()]
    s0, s1, s2 = [int(v) for v in g["noise_split"].tolist()]
    assert s0 == s1          # the generator draws none
    nz = [R.randn(f"{name}.it{it}.noise{i}", s if nb is None else (nb,) + tuple(s[1:]), 2)[rows] for i, s in enumerate(shapes)]
    return (None, None, [n.cuda() for n in nz[s1:s2]])


def spy_grads(st, run):
    calls, orig = [], st.opt.step

    def spy(*a, **kw):
        calls.append(st.w1.grad.detach().clone())
        return orig(*a, **kw)
    st.opt.step = spy
    try:
        r = run()
    finally:
        st.opt.step = orig
    return r, calls


@pytest.mark.parametrize("mode", MODES)
def test_noise_loop_matches_reference_run(mode):
    g = golden("embed_v2_noise.npz")
    st = make_step(optimize_noise=True)
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    st.begin_image(imgs1, w_init=torch.as_tensor(g["w0"]))
    assert all(tuple(m.shape) == (1, r, r) for m, r in zip(st.noise.maps, S2N_RES))          # coupled form: one shared set
    lt = 1e-3 if mode == "det" else 3e-3
    worst = dict(noise=0.0, noise_grad=0.0)
    for it in range(2):
        r, calls = spy_grads(st, lambda: st.step(imgs1, noises=enc_noises(g, it)))
        pre = f"it{it}"
        ngrad = torch.cat([x.reshape(-1) for x in r["noise_grads"]])
        maps = torch.cat([x.reshape(-1) for x in r["noises"]])
        m = dict(w1=relerr(r["w1"], g[f"{pre}_w1"]), w1_l2=l2rel(r["w1"], g[f"{pre}_w1"]), w2=relerr(r["w2"], g[f"{pre}_w2"]),
                 imgs2=relerr(r["imgs2"], g[f"{pre}_imgs2"]), grad1=l2rel(calls[0], g[f"{pre}_grad1"]), grad2=l2rel(calls[1], g[f"{pre}_grad2"]),
                 noise=l2rel(maps, g[f"{pre}_noise"]), noise_grad=l2rel(ngrad, g[f"{pre}_noise_grad"]),
                 reg=abs(float(r["noise_reg"][0]) - float(g[f"{pre}_reg"])) / float(g[f"{pre}_reg"]))
        meas(f"embed_v2_noise.{mode}.it{it}", **m)
        worst = {k: max(v, m[k]) for k, v in worst.items()}
        # the mode-W bounds of test_embed_v2_loop_matches_reference_run, none widened
        assert m["w1_l2"] < 1e-3 and m["w1"] < 4e-3, (it, m)
        assert m["w2"] < (2e-3 if it == 0 else 1e-2), (it, m)
        assert m["imgs2"] < 2e-3, (it, m)
        assert m["grad1"] < (5e-3 if it == 0 else 6e-2) and m["grad2"] < 6e-2, (it, m)
        info = r["info_img"].cpu().numpy()
        got = [float(r["loss_msiv"]), info[0, 0], info[1, 0], info[2, 0], float(r["loss_w"]), 0.0, float(r["norm"]), float(r["loss_mslv"])]
        ref = g[f"{pre}_losses"]
        for k, (a, b) in enumerate(zip(got, ref)):          # loss_msiv stays the image loss alone
            assert abs(a - b) <= (lt if it == 0 else 3 * lt) * abs(b) + 1e-7, (it, k, got, ref.tolist())
        assert m["reg"] <= (lt if it == 0 else 3 * lt), (it, m)
        assert m["noise"] < NOISE_L2_BOUND and m["noise_grad"] < NOISE_GRAD_L2_BOUND, (it, m)
        for x in r["noises"]:          # renormalised
            assert abs(float(x.mean())) < 1e-5 and abs(float((x * x).mean()) - 1) < 1e-5
    meas(f"embed_v2_noise.{mode}.worst", **worst)


def test_independent_rows_equal_single_row_runs():
    """Every row of an independent B = 3 run (a copy of the maps per row) against the batch-1 run of its image, inside the bounds
    test_embed_rows_gpu.check_row applies; the maps of a row inside the bound of the maps above."""
    from dge_amd import ops
    g = golden("embed_v2_noise.npz")
    nb = 3
    imgs = torch.cat((torch.as_tensor(g["imgs1"]), torch.tanh(R.randn("embed_v2_noise.img3", (1, 3, 64, 64), 74, 0.8)))).cuda()
    w0 = R.randn("embed_v2_noise.rows.w0", (nb, 2 * L, 512), 6)
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        st = make_step(optimize_noise=True, independent=True)
        st.begin_image(imgs, w_init=w0)
        assert all(tuple(m.shape) == (nb, r, r) for m, r in zip(st.noise.maps, S2N_RES))
        out = []
        for it in range(2):
            r = st.step(imgs, noises=enc_noises(g, it, "embed_v2_noise.rows", nb=nb))
            out.append({k: ([x.clone() for x in v] if isinstance(v, list) else v.clone() if torch.is_tensor(v) else v) for k, v in r.items()})
        lt = 1e-3
        for b in range(nb):
            one = make_step(optimize_noise=True)
            rows = slice(b, b + 1)
            one.begin_image(imgs[rows], w_init=w0[rows])
            for it in range(2):
                o = one.step(imgs[rows], noises=enc_noises(g, it, "embed_v2_noise.rows", rows, nb))
                got = out[it]
                m = dict(w1=relerr(got["w1"][rows], o["w1"].cpu().numpy()), w1_l2=l2rel(got["w1"][rows], o["w1"].cpu().numpy()),
                         w2=relerr(got["w2"][rows], o["w2"].cpu().numpy()), imgs2=relerr(got["imgs2"][rows], o["imgs2"].cpu().numpy()),
                         noise=l2rel(torch.cat([x[rows].reshape(-1) for x in got["noises"]]), torch.cat([x.reshape(-1) for x in o["noises"]]).cpu().numpy()))
                meas(f"embed_v2_noise.rows.row{b}.it{it}", **m)
                assert m["w1_l2"] < 1e-3 and m["w1"] < 4e-3, (b, it, m)
                assert m["w2"] < (2e-3 if it == 0 else 1e-2) and m["imgs2"] < 2e-3, (b, it, m)
                assert m["noise"] < NOISE_L2_BOUND, (b, it, m)
                for k in ("loss_msiv", "loss_w", "norm", "loss_mslv", "noise_reg"):
                    x, y = float(got[k][b]), float(o[k].reshape(-1)[0])
                    assert abs(x - y) <= (lt if it == 0 else 3 * lt) * abs(y) + 1e-7, (b, it, k, x, y)
        assert len(st.tracker()) == nb
    finally:
        ops.set_deterministic(was)


def test_phase_two_launches_no_noise_pass_and_moves_no_map():
    from dge_amd import ops
    g = golden("embed_v2_noise.npz")
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    st = make_step(optimize_noise=True)
    st.begin_image(imgs1, w_init=torch.as_tensor(g["w0"]))
    start = st.noise.flat.detach().clone()
    seen, orig = [], st._opt_phase

    def phase(loss, retain_graph=False):
        before, n0 = st.noise.flat.detach().clone(), sum(1 for n, _ in log if n == "dge_s2_noise_grad")
        orig(loss, retain_graph=retain_graph)
        seen.append((torch.equal(before, st.noise.flat.detach()), sum(1 for n, _ in log if n == "dge_s2_noise_grad") - n0))
    st._opt_phase = phase
    ops.KERNEL_LOG = log = []
    try:
        st.step(imgs1, noises=enc_noises(g, 0))
    finally:
        ops.KERNEL_LOG = None
    names = [n for n, _ in log]
    # phase 1: one pass per map; phase 2: none, and the maps have the bits they had when it began
    assert seen == [(True, len(S2N_RES)), (True, 0)], seen
    assert names.count("dge_noise_reg") == 1 and names.count("dge_noise_normalize") == 1
    assert not torch.equal(start, st.noise.flat.detach())          # one step per iteration
    assert st.nopt.state[st.noise.flat]["step"] == 1 and st.opt.state[st.w1]["step"] == 2          # a step count of their own
    assert st.G.synthesis.noise_grad_enabled is True
    # begin_image puts the maps back and clears their Adam state, in place
    ptr = st.noise.flat.data_ptr()
    st.begin_image(imgs1, w_init=torch.as_tensor(g["w0"]))
    assert torch.equal(start, st.noise.flat.detach()) and st.noise.flat.data_ptr() == ptr
    assert st.nopt.state[st.noise.flat]["step"] == 0 and float(st.nopt.state[st.noise.flat]["exp_avg_sq"].abs().max()) == 0.0


def test_flag_off_is_the_step_without_the_feature():
    from dge_amd import ops
    g = golden("embed_v2_noise.npz")
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        res = []
        for kw in ({}, dict(optimize_noise=False, noise_reg=3.0, noise_lr=0.5)):
            st = make_step(**kw)
            st.begin_image(imgs1, w_init=torch.as_tensor(g["w0"]))
            ops.KERNEL_LOG = log = []
            try:
                r = st.step(imgs1, noises=enc_noises(g, 0))
            finally:
                ops.KERNEL_LOG = None
            assert "noises" not in r and "noise_reg" not in r
            res.append((r["w1"].clone(), r["imgs2"].clone(), [n for n, _ in log]))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]
        assert not any("noise" in n for n in res[0][2])
    finally:
        ops.set_deterministic(was)


def test_group_files_reload_into_synthesis(tmp_path):
    """finish_group writes models/id{n}-noise.pt, the list of maps of that image; with the saved w1 they are the state the next
    iteration synthesises from: synthesis(noises=...) on them gives that iteration's imgs2 to the bit."""
    from dge_amd import ops
    from dge_amd.embedding_v2 import invert_v2
    g = golden("embed_v2_noise.npz")
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    for sub in ("imgs", "models", "summaries"):
        os.makedirs(tmp_path / sub)
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        st = make_step(optimize_noise=True, independent=True)
        r = invert_v2(st, imgs1, 2, launch="eager", save_every=0, out_dir=str(tmp_path), group=0, w_init=torch.as_tensor(g["w0"]))
        w1 = r["w1"].clone()
        files = [torch.load(tmp_path / "models" / f"id{n}-noise.pt") for n in range(2)]
        for maps in files:
            assert [tuple(m.shape) for m in maps] == [(1, s, s) for s in S2N_RES]
            for m in maps:
                assert abs(float(m.mean())) < 1e-5 and abs(float((m * m).mean()) - 1) < 1e-5
        noises = [torch.cat([files[b][i] for b in range(2)]).cuda() for i in range(len(S2N_RES))]
        with torch.no_grad():
            wt = ops.wplus_lerp(w1, st.G.truncation.w_avg, st.psi)
            img = st.G.synthesis(wt, noises=noises)["image"]
        nxt = st.step(imgs1)
        assert torch.equal(nxt["imgs2"], img)
    finally:
        ops.set_deterministic(was)


def test_noise_replay_equals_eager_bitwise():
    """Deterministic mode: three replays of the captured iteration give the bits of three eager iterations - w1 and the maps (the
    maps, their gradient buffer and the table are static; the maps' optimiser takes its step factor from its own device scalar)."""
    from dge_amd import ops
    g = golden("embed_v2_noise.npz")
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    w0 = torch.as_tensor(g["w0"])
    noises = enc_noises(g, 0)
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        a = make_step(optimize_noise=True)
        a.begin_image(imgs1, w_init=w0)
        a.opt.graph_begin(2, imgs1.device)
        a.nopt.graph_begin(1, imgs1.device)
        ea = []
        for _ in range(3):
            a.opt.graph_advance()
            a.nopt.graph_advance()
            r = a.step(imgs1, noises)
            ea.append((r["w1"].clone(), a.noise.flat.detach().clone()))
        b = make_step(optimize_noise=True)
        b.begin_image(imgs1, w_init=w0)
        b.capture(imgs1, noises, warmup=1)
        b.begin_image(imgs1, w_init=w0)
        rb = []
        for _ in range(3):
            r = b.replay()
            rb.append((r["w1"].clone(), b.noise.flat.detach().clone()))
        torch.cuda.synchronize()
        for i in range(3):
            assert torch.equal(ea[i][0], rb[i][0]) and torch.equal(ea[i][1], rb[i][1]), i
        assert not torch.equal(ea[0][1], ea[2][1])
    finally:
        ops.set_deterministic(was)


def test_cli_run_writes_the_noise_files(tmp_path):
    """python -m dge_amd.embedding_v2 --mtype 2 --optimizeE false --optimize_noise true, three iterations on two 64 x 64 images: the
    usual files plus models/id0-noise.pt and models/id1-noise.pt, maps of zero mean and unit mean square."""
    import subprocess
    import sys
    from tests.conftest import ROOT
    torch.save(torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)), tmp_path / "imgs.pt")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "dge_amd.embedding_v2", "--mtype", "2", "--optimizeE", "false", "--optimize_noise", "true",
                        "--iterations", "3", "--allow_standin_lpips", "--img_size", "64", "--start_features", "16", "--fmaps_base", "2048",
                        "--fmaps_max", "128", "--enc_maxf", "64", "--compute_dtype", "f32", "--img_dir", str(tmp_path / "imgs.pt"),
                        "--experiment_dir", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "group 0:" in r.stdout and "group 1:" in r.stdout
    assert tuple(torch.load(out / "models" / "w_all_1.pt").shape) == (2, 2 * L, 512)
    for n in range(2):
        maps = torch.load(out / "models" / f"id{n}-noise.pt")
        assert [tuple(m.shape) for m in maps] == [(1, s, s) for s in S2N_RES]
        for m in maps:
            assert abs(float(m.mean())) < 1e-5 and abs(float((m * m).mean()) - 1) < 1e-5
