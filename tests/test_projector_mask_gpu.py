"""The masked projection on the GPU (ProjectorStep.begin_image(mask=...), project(mask=...), --mask_dir): three iterations against
the reference loop with the float64 masked distance (tests/golden/projector_mask.npz, tools/gen_golden_projector_mask.py), the
all-ones mask against the unmasked step, independence of what lies under the mask, rows against their batch-1 runs, replay against
eager with a mask per group, and the files.  Helpers and bounds are those of tests/test_projector_gpu.py, as they stand."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import MODES, golden, meas
from tests.projector_mask_models import proj_mask
from tests.projector_models import EXEMPT_CAP, PROJ_B, PROJ_ITERS, exempt_mask, proj_targets, proj_w_noise, split_maps
from tests.test_projector_gpu import (NOISE_GRAD_L2_BOUND, NOISE_L2_BOUND, ROWS_NOISE_L2_BOUND, flat_grads, flat_maps, l2rel, make_step,
                                      relerr, rows_inputs)

pytestmark = pytest.mark.gpu


class deterministic:
    def __enter__(self):
        from dge_amd import ops
        self.was = ops.is_deterministic()
        ops.set_deterministic(True)

    def __exit__(self, *exc):
        from dge_amd import ops
        ops.set_deterministic(self.was)


def three_masks(nb=3):
    """a different mask per row: the fixture's soft edge, a binary half-plane, and a soft random field"""
    m = proj_mask(nb)
    m[1] = (m[1] > 0.5).float()
    m[2] = torch.rand(1, 64, 64, generator=torch.Generator().manual_seed(3)) * 0.9 + 0.1
    return m.cuda().contiguous()


@pytest.mark.parametrize("mode", MODES)
def test_masked_projector_matches_reference_run(mode):
    g, gm = golden("projector.npz"), golden("projector_mask.npz")
    st = make_step()
    st.w_stats(z=torch.as_tensor(g["z"]))
    target, mask = torch.as_tensor(g["target"]).cuda(), torch.as_tensor(gm["mask"]).cuda()
    assert torch.equal(mask.cpu(), proj_mask())
    st.begin_image(target, mask=mask)
    lt = 1e-3 if mode == "det" else 3e-3
    worst = dict(noise=0.0, noise_grad=0.0, w=0.0, w_l2=0.0, w_grad=0.0, dist=0.0, reg=0.0)
    for it in range(PROJ_ITERS):
        pre = f"it{it}"
        r = st.step(target, w_noise=torch.as_tensor(g[f"{pre}_w_noise"]).cuda())
        w, wg = r["w"].cpu().numpy(), r["w_grad"].cpu().numpy()
        maps, grads = flat_maps(r), flat_grads(r)
        share = max(float(exempt_mask(x).mean()) for x in split_maps(gm[f"{pre}_noise_grad"]) + [gm[f"{pre}_w_grad"]])
        m = dict(w=relerr(w, gm[f"{pre}_w"]), w_l2=l2rel(w, gm[f"{pre}_w"]), w_grad=l2rel(wg, gm[f"{pre}_w_grad"]),
                 noise=l2rel(maps, gm[f"{pre}_noise"]), noise_grad=l2rel(grads, gm[f"{pre}_noise_grad"]), exempt=share)
        m["dist"] = float(np.abs(r["dist"].cpu().numpy() / gm[f"{pre}_dist"] - 1).max())
        m["reg"] = float(np.abs(r["reg"].cpu().numpy() / gm[f"{pre}_reg"] - 1).max())
        meas(f"projector_mask.{mode}.it{it}", **m)
        worst = {k: max(v, m[k]) for k, v in worst.items()}
        assert m["w_l2"] < 1e-3 and m["w"] < 4e-3, (it, m)
        assert m["w_grad"] < (5e-3 if it == 0 else 6e-2), (it, m)
        assert m["dist"] <= (lt if it == 0 else 3 * lt) and m["reg"] <= (lt if it == 0 else 3 * lt), (it, m)
        assert m["noise"] < NOISE_L2_BOUND and m["noise_grad"] < NOISE_GRAD_L2_BOUND, (it, m)
        assert share <= EXEMPT_CAP
        cover = r["mask_cover"].cpu().numpy()
        assert np.abs(cover - gm["mask"].mean(axis=(1, 2, 3))).max() < 1e-6
    meas(f"projector_mask.{mode}.worst", **worst)


def test_all_ones_mask_against_the_unmasked_step():
    """m = 1, deterministic mode, three iterations: w, its gradient and the maps inside the rows bounds of
    tests/test_projector_gpu.py (1e-3 for w, 3 x 2.61e-8 for the maps)"""
    target = proj_targets().cuda()
    ones = torch.ones(PROJ_B, 1, 64, 64, device="cuda")
    with deterministic():
        a, b = make_step(seed=2), make_step(seed=2)
        a.begin_image(target)
        b.begin_image(target, mask=ones)
        equal = True
        for it in range(PROJ_ITERS):
            wn = proj_w_noise(it).cuda()
            ra, rb = a.step(target, w_noise=wn), b.step(target, w_noise=wn)
            assert "mask_cover" not in ra and torch.equal(rb["mask_cover"].cpu(), torch.ones(PROJ_B))
            m = dict(w_l2=l2rel(rb["w"].cpu().numpy(), ra["w"].cpu().numpy()), w=relerr(rb["w"].cpu().numpy(), ra["w"].cpu().numpy()),
                     w_grad=l2rel(rb["w_grad"].cpu().numpy(), ra["w_grad"].cpu().numpy()), noise=l2rel(flat_maps(rb), flat_maps(ra)))
            equal = equal and torch.equal(ra["w"], rb["w"]) and torch.equal(a.noise.flat.detach(), b.noise.flat.detach())
            meas(f"projector_mask.ones.it{it}", bits_equal=str(equal), **m)
            assert m["w_l2"] < 1e-3 and m["w"] < 4e-3 and m["w_grad"] < 1e-3, (it, m)
            assert m["noise"] < ROWS_NOISE_L2_BOUND, (it, m)


def test_three_iterations_do_not_see_what_lies_under_the_mask():
    target = proj_targets().cuda()
    mask = (proj_mask() > 0.5).float().cuda()
    hole = (mask == 0).expand(-1, 3, -1, -1)
    other = torch.where(hole, -target.flip(2), target)
    assert not torch.equal(other, target) and bool(hole.any()) and not bool(hole.all())
    with deterministic():
        res = []
        for t in (target, other):
            st = make_step(seed=4)
            st.begin_image(t, mask=mask)
            for _ in range(PROJ_ITERS):
                r = st.step(t)
            res.append((r["w"].clone(), st.noise.flat.detach().clone(), r["dist"].clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_masked_rows_equal_single_row_runs():
    """B = 3 with three different masks against the three batch-1 runs: the bounds of the existing rows test"""
    nb = 3
    imgs, masks = rows_inputs(nb), three_masks(nb)
    with deterministic():
        st = make_step(seed=5)
        st.begin_image(imgs, mask=masks)
        out = []
        for it in range(PROJ_ITERS):
            r = st.step(imgs)
            out.append(dict(w=r["w"].clone(), maps=[x.clone() for x in r["noises"]], dist=r["dist"].clone(), reg=r["reg"].clone()))
        cover = st.last["mask_cover"].clone()
        for b in range(nb):
            one = make_step(seed=5)
            one.begin_image(imgs[b:b + 1], numbers=[b], mask=masks[b:b + 1])
            for it in range(PROJ_ITERS):
                o = one.step(imgs[b:b + 1])
                got = out[it]
                m = dict(w=relerr(got["w"][b:b + 1].cpu().numpy(), o["w"].cpu().numpy()), w_l2=l2rel(got["w"][b:b + 1].cpu().numpy(), o["w"].cpu().numpy()),
                         noise=l2rel(torch.cat([x[b].reshape(-1) for x in got["maps"]]).cpu().numpy(), flat_maps(o)),
                         dist=abs(float(got["dist"][b]) / float(o["dist"][0]) - 1), reg=abs(float(got["reg"][b]) / float(o["reg"][0]) - 1))
                meas(f"projector_mask.rows.row{b}.it{it}", **m)
                assert m["w_l2"] < 1e-3 and m["w"] < 4e-3, (b, it, m)
                assert m["noise"] < ROWS_NOISE_L2_BOUND, (b, it, m)
                assert m["dist"] <= (1e-3 if it == 0 else 3e-3) and m["reg"] <= (1e-3 if it == 0 else 3e-3), (b, it, m)
            assert torch.equal(o["mask_cover"], cover[b:b + 1])


def test_masked_replay_equals_eager_bitwise_with_a_mask_per_group():
    imgs, masks = rows_inputs(3), three_masks(3)
    a_img, b_img, a_m, b_m = imgs[:2].contiguous(), imgs[1:].contiguous(), masks[:2].contiguous(), masks[1:].contiguous()
    with deterministic():
        def eager(target, mask, numbers):
            st = make_step(seed=3)
            st.begin_image(target, numbers=numbers, mask=mask)
            res = []
            for _ in range(PROJ_ITERS):
                r = st.step(target)
                res.append((r["w"].clone(), st.noise.flat.detach().clone(), r["dist"].clone()))
            return res, r["mask_cover"].clone()
        (ea, ca), (eb, cb) = eager(a_img, a_m, [0, 1]), eager(b_img, b_m, [7, 8])
        st = make_step(seed=3)
        st.begin_image(a_img, numbers=[0, 1], mask=a_m)
        st.capture(a_img, warmup=1)
        for target, mask, numbers, want, cover in ((a_img, a_m, [0, 1], ea, ca), (b_img, b_m, [7, 8], eb, cb)):
            st.begin_image(target, numbers=numbers, mask=mask)
            st.set_image(target, mask=mask)
            for i in range(PROJ_ITERS):
                r = st.replay()
                torch.cuda.synchronize()
                assert torch.equal(r["w"], want[i][0]) and torch.equal(st.noise.flat.detach(), want[i][1]), (numbers, i)
                assert torch.equal(r["dist"], want[i][2]) and torch.equal(r["mask_cover"], cover), (numbers, i)
        assert not torch.equal(ea[2][0], eb[2][0])
        # a masked capture refuses a group without a mask, and an unmasked capture a group with one
        with pytest.raises(ValueError, match="captured with a mask"):
            st.begin_image(a_img, numbers=[0, 1])
        plain = make_step(seed=3)
        plain.begin_image(a_img, numbers=[0, 1])
        plain.capture(a_img, warmup=1)
        with pytest.raises(ValueError, match="captured without a mask"):
            plain.begin_image(a_img, numbers=[0, 1], mask=a_m)
        with pytest.raises(ValueError, match="captured without a mask"):
            plain.set_image(a_img, mask=a_m)


def cli(tmp_path, out, extra):
    from dge_amd.projector import main
    return main(["--steps", "3", "--batch_size", "2", "--allow_standin_lpips", "--img_size", "64", "--fmaps_base", "2048", "--fmaps_max", "128",
                 "--compute_dtype", "f32", "--w_avg_samples", "64", "--save_every", "1", "--img_dir", str(tmp_path / "imgs.pt"),
                 "--experiment_dir", str(out), "--deterministic", "true"] + extra)


def test_cli_run_with_masks_writes_blend_and_mask_files(tmp_path):
    """--mask_dir with a folder of 8-bit masks on a [3,3,64,64] .pt, batch 2 (a padded second group): blend/*.png holds the bytes of
    the host formula on the sources of real/ and rec/, mask/*.png gives the mask files back; a run without the flag writes no new
    file and no new Loss.txt field."""
    from PIL import Image
    from dge_amd import ops
    from dge_amd.infer import quantize_u8
    N = 3
    imgs = torch.rand(N, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    torch.save(imgs, tmp_path / "imgs.pt")
    os.makedirs(tmp_path / "masks")
    m8 = (three_masks(N).cpu()[:, 0] * 255).round().to(torch.uint8)
    for n in range(N):
        Image.fromarray(m8[n].numpy()).save(tmp_path / "masks" / f"m{n}.png")
    was = ops.is_deterministic()
    try:
        out = tmp_path / "out"
        st = cli(tmp_path, out, ["--mask_dir", str(tmp_path / "masks")])
        assert st.captured and st.group == 1
        real = imgs.cuda() * 2 - 1
        masks = (m8.float() / 255.0)[:, None]
        for n in range(N):
            wp, maps = (torch.load(out / "models" / f"id{n}-{k}.pt") for k in ("wp", "noise"))
            with torch.no_grad():
                rec = st.G.synthesis(wp.cuda(), noises=[x.cuda() for x in maps])["image"].float()
            assert np.array_equal(np.asarray(Image.open(out / "rec" / f"{n:05d}.png")), quantize_u8(rec)[0].cpu().numpy())
            m = masks[n:n + 1]
            host = (m * real[n:n + 1].cpu() + (1 - m) * rec.cpu()).cuda()
            blend = np.asarray(Image.open(out / "blend" / f"{n:05d}.png"))
            assert blend.shape == (64, 64, 3) and np.array_equal(blend, quantize_u8(host)[0].cpu().numpy())
            back = Image.open(out / "mask" / f"{n:05d}.png")
            assert back.mode == "L" and np.array_equal(np.asarray(back), m8[n].numpy())
        assert sorted(os.listdir(out / "blend")) == sorted(os.listdir(out / "mask")) == [f"{n:05d}.png" for n in range(N)]
        lines = open(out / "Loss.txt").read().splitlines()
        assert len(lines) == 9 and all(ln.split()[-2] == "cover:" for ln in lines)
        covers = {int(ln.split("_")[1]): float(ln.split()[-1]) for ln in lines}
        assert all(abs(covers[n] - float(masks[n].mean())) < 1e-6 for n in range(N))
        # ---- without the flag: what the command wrote before
        out2 = tmp_path / "out2"
        cli(tmp_path, out2, [])
        assert sorted(os.listdir(out2)) == ["Loss.txt", "models", "real", "rec"]
        assert all("cover" not in ln and ln.split()[-2] == "noise_scale:" for ln in open(out2 / "Loss.txt").read().splitlines())
    finally:
        ops.set_deterministic(was)
