"""dge_amd.projector.ProjectorStep on the GPU: three iterations against the loop composed from the reference's generator,
torch.optim.Adam, the regulariser and the LPIPS restatement (tests/golden/projector.npz, tools/gen_golden_projector.py); independent
rows against their batch-1 runs; graph replay against eager to the bit; what a projector run leaves of the generator; the files of
the command line."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import MODES, golden, meas
from tests.projector_models import (EXEMPT_CAP, PROJ_B, PROJ_ITERS, PROJ_KW, PROJ_SETTINGS, exempt_mask, proj_state_dict, proj_targets,
                                     split_maps)
from tests.s2_noise_models import S2N_RES

pytestmark = pytest.mark.gpu

# The maps and their gradients against the reference loop, relative L2.  tests/test_embed_v2_noise_gpu.py states 3 * 2.61e-8 for
# the maps and 3 * 1.84e-7 for their gradients.  The gradients' bound holds here as it stands (5.18e-7 measured).  The maps' does
# not: 2.10e-7 was measured against the fixture on the MI355X (worst of the three iterations and both modes; README, "StyleGAN2
# projector"), and the bound is 3x that.  Cause: that loop steps the maps with lr 0.005, this one with 0.1, so the same relative
# error of a gradient moves a map twenty times as far (the first iteration, whose lr is 0 and which only renormalises, measures
# 8.6e-8).
NOISE_L2_BOUND = 3 * 2.10e-7
NOISE_GRAD_L2_BOUND = 3 * 1.84e-7
# The maps of a row of a batch against its batch-1 run: the rows bound of tests/test_embed_v2_noise_gpu.py, as stated there
# (9.6e-9 measured here)
ROWS_NOISE_L2_BOUND = 3 * 2.61e-8
# w_avg (of its largest element) and w_std (relative) against the fixture's CPU f32 mapping and float64 statistics: 3x the values
# measured on the MI355X, 2.29e-7 and 6.1e-9 - but w_std is one f32 number, and no bound on it can sit below one rounding of
# f32 (2^-23 = 1.2e-7), which is therefore its bound.  noise_scale = w_std x a host double, and the fixture stores it rounded to
# f32: w_std's bound plus half a rounding.
W_AVG_BOUND = 3 * 2.29e-7
W_STD_BOUND = 1.2e-7
NOISE_SCALE_BOUND = W_STD_BOUND + 6e-8


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def l2rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def make_step(seed=0, **kw):
    import dge_amd
    from dge_amd.lpips import LPIPS
    from dge_amd.projector import ProjectorStep
    from oracle import lpips_ref as LR
    G = dge_amd.StyleGAN2Generator(64, compute_dtype="f32", **PROJ_KW).cuda()
    G.load_state_dict(proj_state_dict())
    G.eval()
    LP = LPIPS(compute_dtype="f32").cuda()
    LP.load_state_dict(LR.seeded_params(0))
    return ProjectorStep(G, LP, seed=seed, **{**PROJ_SETTINGS, **kw})


def flat_maps(r):
    return torch.cat([x.reshape(-1) for x in r["noises"]]).cpu().numpy()


def flat_grads(r):
    return torch.cat([x.reshape(-1) for x in r["noise_grads"]]).cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
def test_projector_matches_reference_run(mode):
    g = golden("projector.npz")
    st = make_step()
    w_avg, w_std = st.w_stats(z=torch.as_tensor(g["z"]))
    m = dict(w_avg=relerr(w_avg.cpu().numpy(), g["w_avg"]), w_std=abs(w_std - float(g["w_std"])) / float(g["w_std"]))
    meas(f"projector.{mode}.w_stats", **m)
    assert m["w_avg"] < W_AVG_BOUND and m["w_std"] < W_STD_BOUND, m
    target = torch.as_tensor(g["target"]).cuda()
    st.begin_image(target)
    assert tuple(st.w.shape) == (PROJ_B, 512) and all(tuple(x.shape) == (PROJ_B, r, r) for x, r in zip(st.noise.maps, S2N_RES))
    assert torch.equal(st.w[0], st.w_avg) and torch.equal(st.w[1], st.w_avg)
    lt = 1e-3 if mode == "det" else 3e-3
    worst = dict(noise=0.0, noise_grad=0.0, exempt=0.0)
    for it in range(PROJ_ITERS):
        pre = f"it{it}"
        r = st.step(target, w_noise=torch.as_tensor(g[f"{pre}_w_noise"]).cuda())
        assert abs(r["lr"] - float(g[f"{pre}_lr"])) <= 1e-12
        assert abs(r["noise_scale"] - float(g[f"{pre}_noise_scale"])) <= NOISE_SCALE_BOUND * float(g[f"{pre}_noise_scale"])
        w, wg = r["w"].cpu().numpy(), r["w_grad"].cpu().numpy()
        maps, grads = flat_maps(r), flat_grads(r)
        masks = [exempt_mask(x) for x in split_maps(g[f"{pre}_noise_grad"])]          # per tensor Adam steps: every map, and w
        keep = ~np.concatenate([x.ravel() for x in masks])
        share = max(float(x.mean()) for x in masks + [exempt_mask(g[f"{pre}_w_grad"])])
        m = dict(w=relerr(w, g[f"{pre}_w"]), w_l2=l2rel(w, g[f"{pre}_w"]), w_grad=l2rel(wg, g[f"{pre}_w_grad"]),
                 noise=l2rel(maps, g[f"{pre}_noise"]), noise_grad=l2rel(grads, g[f"{pre}_noise_grad"]),
                 noise_kept=l2rel(maps[keep], g[f"{pre}_noise"][keep]), noise_max=relerr(maps, g[f"{pre}_noise"]), exempt=share)
        dist, reg = r["dist"].cpu().numpy(), r["reg"].cpu().numpy()
        m["dist"] = float(np.abs(dist / g[f"{pre}_dist"] - 1).max())
        m["reg"] = float(np.abs(reg / g[f"{pre}_reg"] - 1).max())
        meas(f"projector.{mode}.it{it}", **m)
        worst = {k: max(v, m[k]) for k, v in worst.items()}
        # the mode-W bounds of tests/test_embed_v2_noise_gpu.py for the latent, its gradient and the losses, none widened
        assert m["w_l2"] < 1e-3 and m["w"] < 4e-3, (it, m)
        assert m["w_grad"] < (5e-3 if it == 0 else 6e-2), (it, m)
        assert m["dist"] <= (lt if it == 0 else 3 * lt) and m["reg"] <= (lt if it == 0 else 3 * lt), (it, m)
        assert m["noise"] < NOISE_L2_BOUND and m["noise_grad"] < NOISE_GRAD_L2_BOUND, (it, m)
        assert share <= EXEMPT_CAP
        for x in r["noises"]:          # renormalised, every row
            assert float(x.mean(dim=(1, 2)).abs().max()) < 1e-5 and float(((x * x).mean(dim=(1, 2)) - 1).abs().max()) < 1e-5
        assert tuple(r["ws"].shape) == (PROJ_B, 10, 512) and tuple(r["imgs"].shape) == (PROJ_B, 3, 64, 64)
    assert torch.equal(torch.as_tensor(g["it0_w"]), torch.as_tensor(g["w_avg"]).expand(PROJ_B, -1))          # lr_0 = 0: w stays
    meas(f"projector.{mode}.worst", **worst)


def rows_inputs(nb=3):
    """nb images scaled apart, so that rows that leaked into each other would show"""
    t = proj_targets()
    imgs = torch.cat([t, t[:1].flip(3)]) * torch.tensor([1.0, 0.6, 0.3]).view(nb, 1, 1, 1)
    return imgs.cuda().contiguous()


def test_independent_rows_equal_single_row_runs():
    """A B = 3 group against the three batch-1 runs of its images (the drawn w noise: a function of seed, image number and
    iteration), inside the rows bounds of tests/test_embed_rows_gpu.py (w) and of tests/test_embed_v2_noise_gpu.py (the maps)."""
    from dge_amd import ops
    nb = 3
    imgs = rows_inputs(nb)
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        st = make_step(seed=5)
        st.begin_image(imgs)
        assert st.numbers == [0, 1, 2]
        out = []
        for it in range(PROJ_ITERS):
            r = st.step(imgs)
            out.append(dict(w=r["w"].clone(), ws=r["ws"].clone(), maps=[x.clone() for x in r["noises"]], dist=r["dist"].clone(), reg=r["reg"].clone()))
        assert not torch.equal(out[0]["ws"][0], out[0]["ws"][1])          # every row draws its own noise
        for b in range(nb):
            one = make_step(seed=5)
            one.begin_image(imgs[b:b + 1], numbers=[b])
            for it in range(PROJ_ITERS):
                o = one.step(imgs[b:b + 1])
                got = out[it]
                if it == 0:          # the same start and the same draw
                    assert torch.equal(got["ws"][b:b + 1], o["ws"])
                m = dict(w=relerr(got["w"][b:b + 1].cpu().numpy(), o["w"].cpu().numpy()), w_l2=l2rel(got["w"][b:b + 1].cpu().numpy(), o["w"].cpu().numpy()),
                         noise=l2rel(torch.cat([x[b].reshape(-1) for x in got["maps"]]).cpu().numpy(), flat_maps(o)),
                         dist=abs(float(got["dist"][b]) / float(o["dist"][0]) - 1), reg=abs(float(got["reg"][b]) / float(o["reg"][0]) - 1))
                meas(f"projector.rows.row{b}.it{it}", **m)
                assert m["w_l2"] < 1e-3 and m["w"] < 4e-3, (b, it, m)
                assert m["noise"] < ROWS_NOISE_L2_BOUND, (b, it, m)
                assert m["dist"] <= (1e-3 if it == 0 else 3e-3) and m["reg"] <= (1e-3 if it == 0 else 3e-3), (b, it, m)
    finally:
        ops.set_deterministic(was)


def test_replay_equals_eager_bitwise_and_serves_a_second_group():
    """Deterministic mode: three replays of the captured iteration give the bits of three eager iterations, w and the maps, while
    lr and noise_scale move; set_image + begin_image run a second group on the same graph."""
    from dge_amd import ops
    imgs = rows_inputs(3)
    a_img, b_img = imgs[:2].contiguous(), imgs[1:].contiguous()
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        def eager(target, numbers):
            st = make_step(seed=3)
            st.begin_image(target, numbers=numbers)
            res = []
            for _ in range(PROJ_ITERS):
                r = st.step(target)
                res.append((r["w"].clone(), st.noise.flat.detach().clone(), r["lr"], r["noise_scale"]))
            return res
        ea, eb = eager(a_img, [0, 1]), eager(b_img, [7, 8])
        st = make_step(seed=3)
        st.begin_image(a_img, numbers=[0, 1])
        with pytest.raises(ValueError, match="warmup"):
            st.capture(a_img, warmup=0)
        assert not st.captured
        st.capture(a_img, warmup=1)
        for target, numbers, want in ((a_img, [0, 1], ea), (b_img, [7, 8], eb)):
            st.set_image(target)
            st.begin_image(target, numbers=numbers)
            for i in range(PROJ_ITERS):
                r = st.replay()
                torch.cuda.synchronize()
                assert torch.equal(r["w"], want[i][0]) and torch.equal(st.noise.flat.detach(), want[i][1]), (numbers, i)
                assert r["lr"] == want[i][2] and r["noise_scale"] == want[i][3]
            assert st.it == PROJ_ITERS and st.opt.t == PROJ_ITERS
        assert ea[1][2] != ea[0][2] and ea[1][3] != ea[0][3]          # the schedule moved between the iterations
        assert not torch.equal(ea[2][0], eb[2][0])
    finally:
        ops.set_deterministic(was)


def test_bare_synthesis_is_untouched_by_a_projector_run():
    """G.synthesis(ws) without `noises`, before and after a projector run: the same launches and the same bits."""
    from dge_amd import ops
    st = make_step()
    G = st.G
    ws = torch.as_tensor(golden("projector.npz")["w_avg"]).cuda().reshape(1, 1, 512).repeat(2, 10, 1).contiguous()
    was = ops.is_deterministic()
    ops.set_deterministic(True)

    def bare():          # -> image, KERNEL_LOG names, the conv launches' shape tags (ops.PROFILE: every conv-family launch)
        ops.KERNEL_LOG, ops.PROFILE = log, prof = [], []
        try:
            with torch.no_grad():
                img = G.synthesis(ws)["image"].clone()
        finally:
            ops.KERNEL_LOG = ops.PROFILE = None
        return img, ([n for n, _ in log], [e[3] for e in prof])
    try:
        bare()          # (the first call packs the weights)
        img0, log0 = bare()
        target = proj_targets().cuda()
        st.begin_image(target)
        for _ in range(2):
            st.step(target)
        img1, log1 = bare()
    finally:
        ops.set_deterministic(was)
    assert log0 == log1 and len(log0[1]) > 0
    assert torch.equal(img0, img1)
    assert not any(p.requires_grad for p in G.parameters())


def test_cli_run_writes_files_that_reproduce_the_image(tmp_path):
    """main() with --steps 3 --batch_size 2 on a [3,3,64,64] .pt - a captured first group, a second group on the same graph through
    set_image, short by one image and padded: the files of the module docstring for the three images and none for the padded row;
    id*-wp.pt and id*-noise.pt reloaded into synthesis give rec/*.png byte for byte, and real/*.png holds the input's bytes."""
    from PIL import Image
    from dge_amd import ops
    from dge_amd.infer import quantize_u8
    from dge_amd.projector import main
    N = 3
    imgs = torch.rand(N, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    torch.save(imgs, tmp_path / "imgs.pt")
    out = tmp_path / "out"
    was = ops.is_deterministic()
    try:
        st = main(["--steps", "3", "--batch_size", "2", "--allow_standin_lpips", "--img_size", "64", "--fmaps_base", "2048", "--fmaps_max", "128",
                   "--compute_dtype", "f32", "--w_avg_samples", "64", "--save_every", "1", "--img_dir", str(tmp_path / "imgs.pt"),
                   "--experiment_dir", str(out), "--deterministic", "true"])
        assert st.captured and st.it == 3 and st.group == 1 and st.numbers == [2, 2]          # the short group repeats its last image
        real = quantize_u8((imgs * 2 - 1).cuda()).cpu().numpy()
        recs = []
        for n in range(N):
            w, wp, maps = (torch.load(out / "models" / f"id{n}-{k}.pt") for k in ("w", "wp", "noise"))
            assert tuple(w.shape) == (1, 512) and tuple(wp.shape) == (1, 10, 512)
            assert torch.equal(wp, w.unsqueeze(1).expand(1, 10, 512))
            assert [tuple(x.shape) for x in maps] == [(1, s, s) for s in S2N_RES]
            with torch.no_grad():
                img = st.G.synthesis(wp.cuda(), noises=[x.cuda() for x in maps])["image"]
            rec = np.asarray(Image.open(out / "rec" / f"{n:05d}.png"))
            assert rec.shape == (64, 64, 3) and np.array_equal(rec, quantize_u8(img)[0].cpu().numpy())
            assert np.array_equal(np.asarray(Image.open(out / "real" / f"{n:05d}.png")), real[n])
            recs.append(rec)
        assert not np.array_equal(recs[0], recs[2]) and not np.array_equal(recs[1], recs[2])          # the second group ran on its own image
        lines = open(out / "Loss.txt").read().splitlines()
        assert [ln.split()[0] for ln in lines] == [f"id_{n}_____i_{i}" for i in range(3) for n in (0, 1)] + [f"id_2_____i_{i}" for i in range(3)]
        assert sorted(os.listdir(out / "models")) == sorted(f"id{n}-{k}.pt" for n in range(N) for k in ("w", "wp", "noise"))
        assert sorted(os.listdir(out / "rec")) == sorted(os.listdir(out / "real")) == [f"{n:05d}.png" for n in range(N)]
    finally:
        ops.set_deterministic(was)
