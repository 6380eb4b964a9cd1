"""PGGAN real-image inversion (dge_amd.embedding_v2_pggan): two iterations of mode E and mode W against the loop run on the
reference's own modules (tests/golden/embed_v2_pg.npz, tools/gen_golden_embed_pg.py), graph replay against eager, the independent
rows form against batch-1 runs, and a done-when run of the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import MODES, ROOT, golden, meas
from tests.golden import recipe as R
from tests.test_embed_v2_gpu import l2rel, relerr
from tests.test_encvar import pg_params
from oracle import lpips_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make_models(cd="f32"):
    from dge_amd.encoder_variants import PGBE
    from dge_amd.lpips import LPIPS
    from dge_amd.pggan_generator import PGGANGenerator
    G = PGGANGenerator(64, fmaps_base=1024, fmaps_max=64, compute_dtype=cd).cuda()
    G.load_state_dict({k: (R.randn("pgstep." + k, tuple(v.shape), 51, 0.2 if k.endswith("bias") else 1.0) if v.ndim else v.clone())
                       for k, v in G.state_dict().items()})
    E = PGBE(startf=32, maxf=512, layer_count=5, pggan=True, compute_dtype=cd).cuda()
    E.load_state_dict(pg_params(E))
    LP = LPIPS(compute_dtype=cd).cuda()
    LP.load_state_dict(LR.seeded_params(0))
    return G, E, LP


def case_noises(g, mode, it, rows=None):
    """(E(imgs1), G, E(imgs2)) noise lists of iteration `it` of a golden case; `rows`: that slice of the batch."""
    shapes = [tuple(s) for s in g[f"{mode}_noise_shapes"].tolist()]
    s0, s1 = [int(v) for v in g[f"{mode}_noise_split"].tolist()]
    nz = [R.randn(f"embed_v2_pg.{mode}.it{it}.noise{i}", s, 2) for i, s in enumerate(shapes)]
    if rows is not None:
        nz = [n[rows].contiguous() for n in nz]
    return ([n.cuda() for n in nz[:s0]] or None, None, [n.cuda() for n in nz[s0:s1]])


def init_noises(g, rows=None):
    nz = [R.randn(f"embed_v2_pg.W.init.noise{i}", tuple(s), 2) for i, s in enumerate(g["W_init_noise_shapes"].tolist())]
    return [(n if rows is None else n[rows].contiguous()).cuda() for n in nz]


def begin(st, g, mode, imgs1, rows=None):
    if mode == "W":
        st.begin_image(imgs1, noises=init_noises(g, rows))
    else:
        st.begin_image(imgs1)


STEP_LR = 0.005
PNAMES = ("decode_block.0.conv_1.weight", "decode_block.2.conv_2.weight", "decode_block.1.conv_3.weight",
          "decode_block.1.instance_norm_3.weight", "decode_block.1.bias_1", "FromRGB.from_rgb.weight", "new_final.bias")
# Bounds: those of tests/test_embed_v2_gpu.py::test_embed_v2_loop_matches_reference_run on the same quantities (z in w1's place),
# except in mode E's iteration 1, where they are exceeded and the bound is 3x the measured value (f32, one MI355X).
# Cause: iteration 1 follows two LREQAdam steps with beta_1 = 0 at lr 0.005 on every encoder parameter.  The first step of an
# element is lr * sign(g) whatever |g| is, so an element whose phase-1 gradient is within rounding of zero steps the other way
# than in the reference's run, 2 * lr apart.  Iteration 0 agrees to 3e-6 in z and 1e-6 in the losses; the sampled parameters agree
# to 0.35 * lr after it and to 0.95 * lr after iteration 1 (asserted below at 4.2 * lr per iteration, the BigGAN test's check).
# The effect is discrete: 24 runs in the default (atomics) mode, where the reduction order changes from run to run, fall on four
# levels of the relative L2 of z - 2.5e-4 (2 runs), 4.5e-4 (3), 9.5e-4 (15) and 2.19e-3 (4 runs).  The deterministic mode gives
# 9.4e-4 on every run.
#                            deterministic: measured    bound      atomics: worst of 24 runs   bound
#   z (max)                                8.60e-4    1e-3 (kept)          6.41e-3             1.9e-2
#   imgs2 (max)                            3.85e-3    1.2e-2               1.04e-2             3.1e-2
#   grad of FromRGB weight, phase 1        0.0892     0.27                 0.0969              0.29
#   grad of FromRGB weight, phase 2        0.1000     0.30                 0.153               0.46
# w2 (2.8e-3 / 9.0e-3) and the losses (1.6e-4 / 1.9e-4) stay inside the original 1e-2 and 3 * lt.
Z_BOUND_E_IT1 = {"det": 1e-3, "atomics": 1.9e-2}
IMGS2_BOUND = {"W": {m: (2e-3, 2e-3) for m in ("det", "atomics")}, "E": {"det": (2e-3, 1.2e-2), "atomics": (2e-3, 3.1e-2)}}
GRAD_BOUND = {"W": {m: ((5e-3, 6e-2), (6e-2, 6e-2)) for m in ("det", "atomics")},
              "E": {"det": ((5e-3, 6e-2), (0.27, 0.30)), "atomics": ((5e-3, 6e-2), (0.29, 0.46))}}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("opt", ["E", "W"])
def test_embed_v2_pg_loop_matches_reference_run(opt, mode):
    from dge_amd.embedding_v2_pggan import PGEmbedStep
    g = golden("embed_v2_pg.npz")
    G, E, LP = make_models()
    st = PGEmbedStep(G, E, LP, mode=opt, lr=0.005)
    assert st.beta == 1e-3 and st.norm_p == 2 and st.rules["arm_iter"] == 750
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    begin(st, g, opt, imgs1)
    if opt == "W":
        assert relerr(st.w1, g["W_z0"]) < 1e-3
    lt = 1e-3 if mode == "det" else 3e-3
    for it in range(2):
        calls = []
        orig = st.opt.step

        def spy(*a, **kw):
            calls.append((E.FromRGB.from_rgb.weight.grad if opt == "E" else st.w1.grad).detach().clone())
            return orig(*a, **kw)
        st.opt.step = spy
        try:
            r = st.step(imgs1, noises=case_noises(g, opt, it))
        finally:
            st.opt.step = orig
        pre = f"{opt}_it{it}"
        e_z, e_w2, e_img = relerr(r["w1"], g[f"{pre}_z"]), relerr(r["w2"], g[f"{pre}_w2"]), relerr(r["imgs2"], g[f"{pre}_imgs2"])
        g1, g2 = l2rel(calls[0], g[f"{pre}_grad1"]), l2rel(calls[1], g[f"{pre}_grad2"])
        info = r["info_img"].cpu().numpy()
        got = [float(r["loss_msiv"]), info[0, 0], info[1, 0], info[2, 0], float(r["loss_w"]), float(r["norm"]), float(r["loss_mslv"])]
        ref = g[f"{pre}_losses"]
        worst = max(abs(a - b) / abs(b) for a, b in zip(got, ref))
        meas(f"embed_v2_pg.{opt}.{mode}.it{it}", z=e_z, z_l2=l2rel(r["w1"], g[f"{pre}_z"]), w2=e_w2, imgs2=e_img, grad1=g1, grad2=g2,
             losses=worst)
        assert r["const2"] is None and r["const3"] is None and r["loss_c1"] is None
        if opt == "W":
            assert l2rel(r["w1"], g[f"{pre}_z"]) < 1e-3 and e_z < 4e-3, (it, e_z)
        else:
            assert e_z < (1e-3 if it == 0 else Z_BOUND_E_IT1[mode]), (it, e_z)
        assert e_w2 < (2e-3 if it == 0 else 1e-2), (it, e_w2)
        assert e_img < IMGS2_BOUND[opt][mode][it], (it, e_img)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert abs(a - b) <= (lt if it == 0 else 3 * lt) * abs(b) + 1e-7, (it, k, got, ref.tolist())
        assert g1 < GRAD_BOUND[opt][mode][it][0] and g2 < GRAD_BOUND[opt][mode][it][1], (it, g1, g2)
        if opt == "E":
            ck = R.checksum({k: v.cpu() for k, v in E.state_dict().items()})
        else:
            ck = R.checksum({"z": st.w1.detach().cpu()})
        assert abs(ck - float(g[f"{pre}_param_checksum"])) < 2e-4 * float(g[f"{pre}_param_checksum"])
        if opt == "E":
            sd = E.state_dict()
            flips = {}
            for k in PNAMES:
                ref = torch.as_tensor(g[f"{pre}_after_phase2:{k}"])
                mine = sd[k].cpu()
                assert abs(float(mine.norm()) - float(g[f"{pre}_after_phase2_norm:{k}"])) < 1e-3 * float(g[f"{pre}_after_phase2_norm:{k}"]), (it, k)
                mine = mine if mine.numel() <= 4096 else mine.flatten()[:4096]
                d = (mine - ref.reshape(mine.shape)).abs()
                flips[k] = (float(d.max()), int((d > STEP_LR).sum()), d.numel())
            meas(f"embed_v2_pg.E.{mode}.it{it}.params", **{k: v[0] / STEP_LR for k, v in flips.items()})
            # beta1 = 0: a step is lr * sign(g)-like; single elements whose gradient is within rounding of zero step the other way,
            # 2 * lr per phase, and every other element agrees to rounding (tests/test_embed_v2_big_gpu.py's check)
            for k, (dmax, n, tot) in flips.items():
                assert dmax < 4.2 * STEP_LR * (it + 1), (it, k, dmax)


def test_w_mode_freezes_the_encoder_and_runs_the_fused_generator_backward(monkeypatch):
    """Mode W: no weight-gradient launch anywhere in an iteration, every encoder parameter without a gradient, and the generator
    backward goes through ops.pixelnorm_act_bwd."""
    from dge_amd import ops
    from dge_amd.embedding_v2_pggan import PGEmbedStep
    g = golden("embed_v2_pg.npz")
    G, E, LP = make_models()
    st = PGEmbedStep(G, E, LP, mode="W", lr=0.005)
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    begin(st, g, "W", imgs1)

    def boom(*a, **kw):
        raise AssertionError("parameter-gradient launch with a frozen encoder")
    for name in ("conv_wgrad", "conv_wgrad_dots", "fromrgb_bwd", "dense_wgrad", "chan_sum"):
        monkeypatch.setattr(ops, name, boom)
    ops.KERNEL_LOG = log = []
    try:
        r = st.step(imgs1, noises=case_noises(g, "W", 0))
    finally:
        ops.KERNEL_LOG = None
    torch.cuda.synchronize()
    names = [n for n, _ in log]
    assert names.count("in_bwd_fromrgb_img<f32,data>") == 1, names          # phase 2 alone reaches the encoder's image gradient
    assert sum(n.startswith("pixelnorm_act_bwd<f32") for n in names) == 2 * 9, names          # 9 per generator backward, two phases
    assert torch.isfinite(r["w1"]).all() and all(p.grad is None for p in E.parameters())


def test_w_mode_replay_equals_eager_bitwise():
    """Mode W, deterministic mode: 3 replays of the captured iteration give the bits of 3 eager iterations
    (tests/test_embed_v2_gpu.py::test_w_mode_replay_equals_eager_bitwise); E_PG's noise comes from the device seed scalar in both."""
    from dge_amd import ops
    from dge_amd.embedding_v2_pggan import PGEmbedStep
    g = golden("embed_v2_pg.npz")
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    z0 = torch.as_tensor(g["W_z0"])
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        a = PGEmbedStep(*make_models(), mode="W", lr=0.005)
        a.begin_image(imgs1, w_init=z0)
        a.opt.graph_begin(2, imgs1.device)
        ops.noise_seed(5)          # (noise_graph_begin counts the iterations' seeds from the seed in force)
        ops.noise_graph_begin(imgs1.device)
        wa = []
        for i in range(3):
            a.opt.graph_advance()
            ops.noise_graph_seed(i)
            wa.append(a.step(imgs1)["w1"].clone())
        b = PGEmbedStep(*make_models(), mode="W", lr=0.005)
        b.begin_image(imgs1, w_init=z0)
        ops.noise_seed(5)
        b.capture(imgs1, warmup=1)
        b.begin_image(imgs1, w_init=z0)
        b.graph_iteration = 0
        wb = [b.replay()["w1"].clone() for _ in range(3)]
        torch.cuda.synchronize()
        assert not torch.equal(wa[0], wa[1])
        for i in range(3):
            assert torch.equal(wa[i], wb[i]), (i, relerr(wb[i], wa[i].cpu().numpy()))
    finally:
        ops.set_deterministic(was)


def test_independent_rows_equal_single_row_runs():
    """independent=True at B = 3 (mode W, deterministic): every row against the batch-1 coupled run of its image, within
    tests/test_embed_rows_gpu.py's bounds; the coupled B = 3 step is a different computation."""
    from dge_amd import ops
    from dge_amd.embedding_v2_pggan import PGEmbedStep
    g = golden("embed_v2_pg.npz")
    B = 3
    imgs = torch.cat((torch.as_tensor(g["imgs1"]), torch.tanh(R.randn("embed_v2_pg.row2", (1, 3, 64, 64), 74, 0.8)))).cuda()
    z0 = R.randn("embed_v2_pg.rows.z0", (B, 512), 75)
    shapes = [(B,) + tuple(s)[1:] for s in g["W_noise_shapes"].tolist()]
    noises = lambda it, rows=slice(None): (None, None, [R.randn(f"embed_v2_pg.rows.it{it}.noise{i}", s, 2)[rows].contiguous().cuda()
                                                       for i, s in enumerate(shapes)])
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        G, E, LP = make_models()
        st = PGEmbedStep(G, E, LP, mode="W", lr=0.005, independent=True)
        st.begin_image(imgs, w_init=z0)
        out = []
        for it in range(2):
            r = st.step(imgs, noises=noises(it))
            out.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()})
        assert out[0]["loss_msiv"].shape == (B,) and out[0]["norm"].shape == (B,) and out[0]["info_img"].shape == (B, 3, 8)
        assert len(st.tracker()) == B
        lt = 1e-3
        for b in range(B):
            one = PGEmbedStep(G, E, LP, mode="W", lr=0.005)
            one.begin_image(imgs[b:b + 1], w_init=z0[b:b + 1])
            for it in range(2):
                o = one.step(imgs[b:b + 1], noises=noises(it, slice(b, b + 1)))
                m = dict(z=relerr(out[it]["w1"][b:b + 1], o["w1"].cpu().numpy()), z_l2=l2rel(out[it]["w1"][b:b + 1], o["w1"].cpu().numpy()),
                         w2=relerr(out[it]["w2"][b:b + 1], o["w2"].cpu().numpy()), imgs2=relerr(out[it]["imgs2"][b:b + 1], o["imgs2"].cpu().numpy()))
                meas(f"embed_v2_pg.rows.row{b}.it{it}", **m)
                assert m["z_l2"] < 1e-3 and m["z"] < 4e-3, (b, it, m)
                assert m["w2"] < (2e-3 if it == 0 else 1e-2) and m["imgs2"] < 2e-3, (b, it, m)
                for key in ("loss_msiv", "loss_w", "norm", "loss_mslv"):
                    a_, b_ = float(out[it][key][b]), float(o[key])
                    assert abs(a_ - b_) <= (lt if it == 0 else 3 * lt) * abs(b_) + 1e-7, (b, it, key, a_, b_)
        c = PGEmbedStep(G, E, LP, mode="W", lr=0.005)
        c.begin_image(imgs, w_init=z0)
        coupled = float(c.step(imgs, noises=noises(0))["loss_msiv"])
        assert abs(coupled - float(out[0]["loss_msiv"][0])) > 10 * lt * abs(coupled)
    finally:
        ops.set_deterministic(was)


def test_cli_w_mode_run_writes_the_expected_files(tmp_path):
    """python -m dge_amd.embedding_v2_pggan --optimizeE false --iterations 3 --allow_standin_lpips on seeded weights, two 64 x 64
    images in a .pt: imgs/, models/w_all_1.pt [2,512] and Loss.txt."""
    torch.save(torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)), tmp_path / "imgs.pt")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "dge_amd.embedding_v2_pggan", "--optimizeE", "false", "--iterations", "3",
                        "--allow_standin_lpips", "--img_size", "64", "--start_features", "32", "--fmaps_base", "1024", "--fmaps_max", "64",
                        "--compute_dtype", "f32", "--img_dir", str(tmp_path / "imgs.pt"), "--experiment_dir", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "group 0:" in r.stdout and "group 1:" in r.stdout
    w = torch.load(out / "models" / "w_all_1.pt")
    assert tuple(w.shape) == (2, 512) and torch.isfinite(w).all() and not torch.equal(w[0], w[1])
    assert len([n for n in os.listdir(out / "imgs") if n.startswith("id0_ep0-") or n.startswith("id1_ep0-")]) == 2
    txt = (out / "Loss.txt").read_text()
    assert "id_0_____i_0" in txt and "id_1_____i_0" in txt and "loss_w_info" in txt and "loss_imgs_info" in txt
    assert np.isfinite(float(txt.strip().splitlines()[-1].split(": ")[1]))
