"""Mode "Z" of the v2 inversion loop (dge_amd.embedding_v2: z in front of the mapping network is the optimised latent) for StyleGAN2
and StyleGAN1: two iterations against the loop composed from the reference's own modules (tests/golden/embed_v2_z.npz,
tools/gen_golden_s2_mapping.py) inside the mode-W bounds of tests/test_embed_v2_gpu.py, graph replay against eager, independent
rows against their batch-1 runs (the bounds of tests/test_embed_rows_gpu.py), the unchanged mode-W launches and a CLI run."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import MODES, ROOT, golden, meas
from tests.golden import recipe as R
from tests.s2z_models import s2z_state_dict
from tests.test_embed_v2_gpu import l2rel, make_models, relerr

pytestmark = pytest.mark.gpu
GENS = ["sg2", "sg1"]
L = 5


def models(gen):
    """(G, E, LP, Gm): test_embed_v2_gpu.make_models with the StyleGAN2 mapping weights of the fixture; StyleGAN1: the mapping
    network of step_z.npz (seeded weights, truncation centre)."""
    import dge_amd.stylegan1 as S
    G, E, LP = make_models(gen)
    Gm = None
    if gen == "sg2":
        G.load_state_dict(s2z_state_dict())
    else:
        Gm = S.Mapping(num_layers=2 * L).cuda()
        Gm.load_state_dict({k: R.randn("sg1step.m." + k, tuple(v.shape), 44, 0.05 if k.endswith("weight") else 0.01)
                            for k, v in Gm.state_dict().items()})
        Gm.buffer1 = R.randn("sg1step.buffer1", (2 * L, 512), 44, 0.5)
        for p in Gm.parameters():
            p.requires_grad_(False)
    return G, E, LP, Gm


def make_step(gen, **kw):
    from dge_amd.embedding_v2 import LatentEmbedStep
    G, E, LP, Gm = models(gen)
    return LatentEmbedStep(G, E, LP, mode="Z", generator=gen, lr=0.005, Gm=Gm, **kw)


def init_noises(g, gen, rows=slice(None)):
    if gen != "sg1":
        return None
    shapes = [tuple(s) for s in g["sg1_init_noise_shapes"].tolist()]
    return [R.randn(f"embed_v2_z.sg1.init.noise{i}", s, 2)[rows].cuda() for i, s in enumerate(shapes)]


def case_noises(g, gen, it, rows=slice(None), device_only=False):
    """(unused, G, E(imgs2)) noise lists of iteration `it`; `rows`: of those batch rows (the generator's first noise has batch 1)."""
    shapes = [tuple(s) for s in g[f"{gen}_noise_shapes"].tolist()]
    s0, s1, s2 = [int(v) for v in g[f"{gen}_noise_split"].tolist()]
    nz = [R.randn(f"embed_v2_z.{gen}.it{it}.noise{i}", s, 2) for i, s in enumerate(shapes)]
    nz = [n if n.shape[0] == 1 else n[rows] for n in nz]
    gn = [n.cuda() for n in nz[s0:s1]] if device_only else nz[s0:s1]
    return (None, gn or None, [n.cuda() for n in nz[s1:s2]])


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
@pytest.mark.parametrize("gen", GENS)
def test_z_mode_loop_matches_reference_run(gen, mode):
    g = golden("embed_v2_z.npz")
    st = make_step(gen)
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    st.begin_image(imgs1, w_init=torch.as_tensor(g[f"{gen}_z0"]), noises=init_noises(g, gen))
    assert torch.equal(st.w1.detach().cpu(), torch.as_tensor(g[f"{gen}_z0"]))
    lt = 1e-3 if mode == "det" else 3e-3
    for it in range(2):
        r, calls = spy_grads(st, lambda: st.step(imgs1, noises=case_noises(g, gen, it)))
        pre = f"{gen}_it{it}"
        assert tuple(r["w1"].shape) == (2, 512)
        m = dict(z=relerr(r["w1"], g[f"{pre}_z"]), z_l2=l2rel(r["w1"], g[f"{pre}_z"]), wp=relerr(r["wp"], g[f"{pre}_wp"]),
                 wp_new=relerr(r["wp_new"], g[f"{pre}_wp_new"]), w2=relerr(r["w2"], g[f"{pre}_w2"]), imgs2=relerr(r["imgs2"], g[f"{pre}_imgs2"]),
                 grad1=l2rel(calls[0], g[f"{pre}_grad1"]), grad2=l2rel(calls[1], g[f"{pre}_grad2"]))
        meas(f"embed_v2_z.{gen}.{mode}.it{it}", **m)
        # the mode-W bounds of test_embed_v2_loop_matches_reference_run: the latent has taken sign-like Adam steps (lr 0.005)
        assert m["z_l2"] < 1e-3 and m["z"] < 4e-3, (it, m)
        assert m["wp"] < 4e-3 and m["wp_new"] < 4e-3, (it, m)
        assert m["w2"] < (2e-3 if it == 0 else 1e-2), (it, m)
        assert m["imgs2"] < 2e-3, (it, m)
        info = r["info_img"].cpu().numpy()
        got = [float(r["loss_msiv"]), info[0, 0], info[1, 0], info[2, 0], float(r["loss_w"]),
               float(r["loss_c1"]) if r["loss_c1"] is not None else 0.0, float(r["norm"]), float(r["loss_mslv"])]
        ref = g[f"{pre}_losses"]
        for k, (a, b) in enumerate(zip(got, ref)):
            assert abs(a - b) <= (lt if it == 0 else 3 * lt) * abs(b) + 1e-7, (it, k, got, ref.tolist())
        assert (r["const2"] is None) == (gen == "sg2")
        assert m["grad1"] < (5e-3 if it == 0 else 6e-2) and m["grad2"] < 6e-2, (it, m)


@pytest.mark.parametrize("gen", GENS)
def test_z_mode_replay_equals_eager_bitwise(gen):
    """Deterministic mode: three replays of the captured iteration give the bits of three eager iterations (the truncation cache
    of StyleGAN1 is filled by the warm-up iteration; every launch of the mapping and its adjoint is capturable)."""
    from dge_amd import ops
    g = golden("embed_v2_z.npz")
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    z0 = torch.as_tensor(g[f"{gen}_z0"])
    noises = case_noises(g, gen, 0, device_only=True)
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        for kw in ([{}] if gen == "sg1" else [dict(mapping_bwd="one"), dict(mapping_bwd="wide")]):
            a = make_step(gen, **kw)
            a.begin_image(imgs1, w_init=z0, noises=init_noises(g, gen))
            a.opt.graph_begin(2, imgs1.device)
            za = []
            for _ in range(3):
                a.opt.graph_advance()
                za.append(a.step(imgs1, noises)["w1"].clone())
            b = make_step(gen, **kw)
            b.begin_image(imgs1, w_init=z0, noises=init_noises(g, gen))
            b.capture(imgs1, noises, warmup=1)
            b.begin_image(imgs1, w_init=z0, noises=init_noises(g, gen))
            zb = [b.replay()["w1"].clone() for _ in range(3)]
            torch.cuda.synchronize()
            for i in range(3):
                assert torch.equal(za[i], zb[i]), (kw, i, relerr(zb[i], za[i].cpu().numpy()))
            assert not torch.equal(za[0], za[2])
    finally:
        ops.set_deterministic(was)


@pytest.mark.parametrize("gen", GENS)
def test_z_mode_independent_rows_equal_single_row_runs(gen):
    """Every row of an independent B = 3 run against the batch-1 run of its image, inside the bounds test_embed_rows_gpu.check_row
    applies (what one HIP run may differ from another computation of the same quantity)."""
    from dge_amd import ops
    g = golden("embed_v2_z.npz")
    nb = 3
    imgs = torch.cat((torch.as_tensor(g["imgs1"]), torch.tanh(R.randn("embed_v2_z.img3", (1, 3, 64, 64), 74, 0.8)))).cuda()
    z0 = R.randn("embed_v2_z.rows.z0", (nb, 512), 6)
    shapes = [tuple(s) for s in g[f"{gen}_noise_shapes"].tolist()]
    s0, s1, s2 = [int(v) for v in g[f"{gen}_noise_split"].tolist()]
    ini = None
    if gen == "sg1":
        ini = [R.randn(f"embed_v2_z.rows.init{i}", (nb,) + tuple(s[1:]), 2) for i, s in enumerate(g["sg1_init_noise_shapes"].tolist())]

    def noises(it, rows):
        nz = [R.randn(f"embed_v2_z.rows.{gen}.it{it}.noise{i}", ((1,) if s[0] == 1 else (nb,)) + tuple(s[1:]), 2) for i, s in enumerate(shapes)]
        nz = [n if n.shape[0] == 1 else n[rows] for n in nz]
        return (None, nz[s0:s1] or None, [n.cuda() for n in nz[s1:s2]])
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        st = make_step(gen, independent=True)
        st.begin_image(imgs, w_init=z0, noises=None if ini is None else [n.cuda() for n in ini])
        out = []
        for it in range(2):
            r, calls = spy_grads(st, lambda: st.step(imgs, noises=noises(it, slice(None))))
            out.append((dict((k, v.clone() if torch.is_tensor(v) else v) for k, v in r.items()), calls))
        lt = 1e-3
        for b in range(nb):
            one = make_step(gen)
            rows = slice(b, b + 1)
            one.begin_image(imgs[rows], w_init=z0[rows], noises=None if ini is None else [n[rows].cuda() for n in ini])
            for it in range(2):
                o, oc = spy_grads(one, lambda: one.step(imgs[rows], noises=noises(it, rows)))
                got, gc = out[it]
                m = dict(z=relerr(got["w1"][rows], o["w1"].cpu().numpy()), z_l2=l2rel(got["w1"][rows], o["w1"].cpu().numpy()),
                         w2=relerr(got["w2"][rows], o["w2"].cpu().numpy()), imgs2=relerr(got["imgs2"][rows], o["imgs2"].cpu().numpy()))
                assert m["z_l2"] < 1e-3 and m["z"] < 4e-3, (b, it, m)
                assert m["w2"] < (2e-3 if it == 0 else 1e-2) and m["imgs2"] < 2e-3, (b, it, m)
                for k in ("loss_msiv", "loss_w", "norm", "loss_mslv"):
                    x, y = float(got[k][b]), float(o[k])
                    assert abs(x - y) <= (lt if it == 0 else 3 * lt) * abs(y) + 1e-7, (b, it, k, x, y)
                for phase in range(2):
                    e = l2rel(gc[phase][rows], oc[phase].cpu().numpy())
                    m[f"grad{phase + 1}"] = e
                    assert e < (5e-3 if phase == 0 and it == 0 else 6e-2), (b, it, phase, e)
                meas(f"embed_v2_z.rows.{gen}.row{b}.it{it}", **m)
        assert len(st.tracker()) == nb
    finally:
        ops.set_deterministic(was)


@pytest.mark.parametrize("gen", GENS)
def test_w_mode_step_never_reaches_the_z_mode_code(gen, monkeypatch):
    """A mode-W step issues what it issued: with the Z-mode hooks and the mapping adjoint replaced by functions that raise, it runs,
    and its KERNEL_LOG names no mapping adjoint and is the same on a second step object."""
    from dge_amd import ops
    from dge_amd.embedding_v2 import LatentEmbedStep
    g = golden("embed_v2_z.npz")
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()

    def boom(*a, **kw):
        raise AssertionError("mode W reached the mode-Z code")
    for name in ("_wp_of", "_synthesise"):
        monkeypatch.setattr(LatentEmbedStep, name, boom)
    monkeypatch.setattr(ops, "mapping_bwd", boom)
    logs = []
    for _ in range(2):
        G, E, LP = make_models(gen)
        st = LatentEmbedStep(G, E, LP, mode="W", generator=gen, lr=0.005)
        st.begin_image(imgs1, w_init=R.randn("embed_v2_z.w0", (2, 2 * L, 512), 5))
        log = []
        ops.KERNEL_LOG = log
        try:
            r = st.step(imgs1)
        finally:
            ops.KERNEL_LOG = None
        assert torch.isfinite(r["w1"]).all() and "wp" not in r
        logs.append([n for n, _ in log])
    assert logs[0] == logs[1] and len(logs[0]) > 0 and not any("mapping_bwd" in n for n in logs[0])


def test_cli_z_space_run_writes_the_expected_files(tmp_path):
    """python -m dge_amd.embedding_v2 --optimizeE false --space z --mtype 2, three iterations on two 64 x 64 images in a .pt:
    models/z_all_1.pt [2, 512] and the per-row z files."""
    torch.save(torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)), tmp_path / "imgs.pt")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "dge_amd.embedding_v2", "--optimizeE", "false", "--space", "z", "--mtype", "2",
                        "--iterations", "3", "--allow_standin_lpips", "--img_size", "64", "--start_features", "16", "--fmaps_base", "2048",
                        "--fmaps_max", "128", "--enc_maxf", "64", "--compute_dtype", "f32", "--img_dir", str(tmp_path / "imgs.pt"),
                        "--experiment_dir", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "group 0:" in r.stdout and "group 1:" in r.stdout
    z = torch.load(out / "models" / "z_all_1.pt")
    assert tuple(z.shape) == (2, 512) and torch.isfinite(z).all() and not torch.equal(z[0], z[1])
    names = os.listdir(out / "models")
    assert any(n.startswith("id0-i0-z0-") for n in names) and any(n.startswith("id1-i0-z0-") for n in names), names
    assert not any(n.startswith("w_all") for n in names)
