"""dge_amd.projector.StyleProjectorStep on the GPU: three iterations of the S refinement against the loop composed from the
reference's generator (its style modules hooked to leaves), torch.optim.Adam, the regulariser and the LPIPS restatement
(tests/golden/projector_styles.npz, tools/gen_golden_s2_styles.py); replay against eager to the bit and a second group on the same
graph; independent rows against their batch-1 runs; the masked iteration.  B = 2, 64^2, f32.  The bounds are those
tests/test_projector_gpu.py holds for w, its gradient, dist / reg and the maps, as they stand there."""
import numpy as np
import pytest
import torch

from tests.conftest import MODES, golden, meas
from tests.projector_models import EXEMPT_CAP, PROJ_B, PROJ_ITERS, PROJ_KW, exempt_mask, proj_state_dict, split_maps
from tests.s2_style_models import STYLE_SETTINGS, split_blocks
from tests.test_projector_gpu import NOISE_GRAD_L2_BOUND, NOISE_L2_BOUND, ROWS_NOISE_L2_BOUND, l2rel, relerr, rows_inputs

pytestmark = pytest.mark.gpu
_M = {}


def models():
    if not _M:
        import dge_amd
        from dge_amd.lpips import LPIPS
        from oracle import lpips_ref as LR
        G = dge_amd.StyleGAN2Generator(64, compute_dtype="f32", **PROJ_KW).cuda()
        G.load_state_dict(proj_state_dict())
        G.eval()
        LP = LPIPS(compute_dtype="f32").cuda()
        LP.load_state_dict(LR.seeded_params(0))
        _M.update(G=G, LP=LP)
    return _M["G"], _M["LP"]


def make_stage(**kw):
    from dge_amd.projector import StyleProjectorStep
    G, LP = models()
    return StyleProjectorStep(G, LP, **{**STYLE_SETTINGS, **kw})


def start_wp(nb):
    """a start code per row: mapped samples in every row of W+, as the fixture's"""
    from tests.projector_models import proj_z
    G, _ = models()
    with torch.no_grad():
        w = G.mapping(proj_z()[:nb].cuda())["w"].float()
    return w.unsqueeze(1).repeat(1, 10, 1).contiguous()


def flat_maps(r):
    return torch.cat([x.reshape(-1) for x in r["noises"]]).cpu().numpy()


def flat_grads(r):
    return torch.cat([x.reshape(-1) for x in r["noise_grads"]]).cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
def test_style_stage_matches_reference_run(mode):
    """The codes behind each of three iterations, their gradients, dist, reg and the maps.  Elements whose fixture gradient is below
    1e-6 of their tensor's largest (a style block, a map) may step the other way under Adam's first steps; the `kept` figures leave
    them out, at most 0.1 % of a tensor (tests/test_projector_styles_cli.py: the fixture has none in its style blocks).  The bounds
    hold on the whole tensors, so the assertions are made there and the `kept` figures are only reported."""
    g = golden("projector_styles.npz")
    st = make_stage()
    target, wp = torch.as_tensor(g["target"]).cuda(), torch.as_tensor(g["wp"]).cuda()
    st.begin_image(target, wp)
    assert relerr(st.codes.detached().cpu().numpy(), g["styles0"]) < 2e-4          # (the forward bound of the styles, f32)
    assert [tuple(x.shape) for x in st.noise.maps] == [(PROJ_B, r, r) for r in (4, 8, 8, 16, 16, 32, 32, 64, 64)]
    lt = 1e-3 if mode == "det" else 3e-3
    worst = {}
    for it in range(PROJ_ITERS):
        pre = f"it{it}"
        r = st.step(target)
        assert abs(r["lr"] - float(g[f"{pre}_lr"])) <= 1e-12
        s, sg = r["styles"].cpu().numpy(), r["style_grad"].cpu().numpy()
        maps, grads = flat_maps(r), flat_grads(r)
        s_masks = [exempt_mask(x) for x in split_blocks(g[f"{pre}_style_grad"], PROJ_B)]
        n_masks = [exempt_mask(x) for x in split_maps(g[f"{pre}_noise_grad"])]
        s_keep, n_keep = ~np.concatenate([x.ravel() for x in s_masks]), ~np.concatenate([x.ravel() for x in n_masks])
        share = max(float(x.mean()) for x in s_masks + n_masks)
        m = dict(styles=relerr(s, g[f"{pre}_styles"]), styles_l2=l2rel(s, g[f"{pre}_styles"]), style_grad=l2rel(sg, g[f"{pre}_style_grad"]),
                 styles_kept_l2=l2rel(s[s_keep], g[f"{pre}_styles"][s_keep]), styles_kept=relerr(s[s_keep], g[f"{pre}_styles"][s_keep]),
                 noise=l2rel(maps, g[f"{pre}_noise"]), noise_grad=l2rel(grads, g[f"{pre}_noise_grad"]),
                 noise_kept=l2rel(maps[n_keep], g[f"{pre}_noise"][n_keep]), exempt=share)
        dist, reg = r["dist"].cpu().numpy(), r["reg"].cpu().numpy()
        m["dist"] = float(np.abs(dist / g[f"{pre}_dist"] - 1).max())
        m["reg"] = float(np.abs(reg / g[f"{pre}_reg"] - 1).max())
        meas(f"projector_styles.{mode}.it{it}", **m)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in m.items()}
        # the bounds of tests/test_projector_gpu.py for w (here: the codes), its gradient, the losses and the maps, none widened
        assert m["styles_l2"] < 1e-3 and m["styles"] < 4e-3, (it, m)          # (whole tensors: nothing had to be left out)
        assert m["style_grad"] < (5e-3 if it == 0 else 6e-2), (it, m)
        assert m["dist"] <= (lt if it == 0 else 3 * lt) and m["reg"] <= (lt if it == 0 else 3 * lt), (it, m)
        assert m["noise"] < NOISE_L2_BOUND and m["noise_grad"] < NOISE_GRAD_L2_BOUND, (it, m)
        assert share <= EXEMPT_CAP
        for x in r["noises"]:          # renormalised, every row
            assert float(x.mean(dim=(1, 2)).abs().max()) < 1e-5 and float(((x * x).mean(dim=(1, 2)) - 1).abs().max()) < 1e-5
    assert np.array_equal(g["it0_styles"], g["styles0"])          # lr_0 = 0: the codes stay
    meas(f"projector_styles.{mode}.worst", **worst)


def test_style_stage_rows_equal_single_row_runs():
    """A B = 3 group against the three batch-1 runs of its images and start codes, inside the rows bounds of
    tests/test_projector_gpu.py."""
    from dge_amd import ops
    nb = 3
    imgs, wp = rows_inputs(nb), start_wp(nb)
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        st = make_stage()
        st.begin_image(imgs, wp)
        out = []
        for it in range(PROJ_ITERS):
            r = st.step(imgs)
            out.append(dict(rows=[[x.clone() for x in st.codes.rows(b)] for b in range(nb)], maps=[x.clone() for x in r["noises"]],
                            dist=r["dist"].clone(), reg=r["reg"].clone()))
        for b in range(nb):
            one = make_stage()
            one.begin_image(imgs[b:b + 1], wp[b:b + 1].contiguous(), numbers=[b])
            for it in range(PROJ_ITERS):
                o = one.step(imgs[b:b + 1])
                got = out[it]
                a, c = torch.cat(got["rows"][b], 1).cpu().numpy(), torch.cat(one.codes.rows(0), 1).cpu().numpy()
                m = dict(styles=relerr(a, c), styles_l2=l2rel(a, c),
                         noise=l2rel(torch.cat([x[b].reshape(-1) for x in got["maps"]]).cpu().numpy(), flat_maps(o)),
                         dist=abs(float(got["dist"][b]) / float(o["dist"][0]) - 1), reg=abs(float(got["reg"][b]) / float(o["reg"][0]) - 1))
                meas(f"projector_styles.rows.row{b}.it{it}", **m)
                assert m["styles_l2"] < 1e-3 and m["styles"] < 4e-3, (b, it, m)
                assert m["noise"] < ROWS_NOISE_L2_BOUND, (b, it, m)
                assert m["dist"] <= (1e-3 if it == 0 else 3e-3) and m["reg"] <= (1e-3 if it == 0 else 3e-3), (b, it, m)
    finally:
        ops.set_deterministic(was)


def test_style_stage_replay_equals_eager_bitwise_and_serves_a_second_group():
    """Deterministic mode: three replays of the captured iteration give the bits of three eager iterations, codes and maps, while lr
    moves; set_image + begin_image run a second group on the same graph."""
    from dge_amd import ops
    imgs, wp = rows_inputs(3), start_wp(3)
    a_img, b_img, a_wp, b_wp = imgs[:2].contiguous(), imgs[1:].contiguous(), wp[:2].contiguous(), wp[1:].contiguous()
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        def eager(target, wp_):
            st = make_stage()
            st.begin_image(target, wp_)
            res = []
            for _ in range(PROJ_ITERS):
                r = st.step(target)
                res.append((r["styles"].clone(), st.noise.flat.detach().clone(), r["lr"], r["dist"].clone()))
            return res
        ea, eb = eager(a_img, a_wp), eager(b_img, b_wp)
        st = make_stage()
        st.begin_image(a_img, a_wp)
        with pytest.raises(ValueError, match="warmup"):
            st.capture(a_img, warmup=0)
        assert not st.captured
        st.capture(a_img, warmup=1)
        for target, wp_, want in ((a_img, a_wp, ea), (b_img, b_wp, eb)):
            st.set_image(target)
            st.begin_image(target, wp_)
            for i in range(PROJ_ITERS):
                r = st.replay()
                torch.cuda.synchronize()
                assert torch.equal(r["styles"], want[i][0]) and torch.equal(st.noise.flat.detach(), want[i][1]), i
                assert r["lr"] == want[i][2] and torch.equal(r["dist"], want[i][3])
            assert st.it == PROJ_ITERS and st.opt.t == PROJ_ITERS
        assert ea[1][2] != ea[0][2]          # the schedule moved between the iterations
        assert not torch.equal(ea[2][0], eb[2][0])
        with pytest.raises(ValueError, match="different batch"):
            st.begin_image(imgs, wp)
    finally:
        ops.set_deterministic(was)


def test_style_stage_masked_iteration_and_shared_maps():
    """The mask path: a captured masked iteration equals the eager masked iteration to the bit (deterministic mode), differs from the
    unmasked one, and reports the cover; a NoiseMaps given to begin_image is refined in place, not reset."""
    from dge_amd import ops
    from dge_amd.noise_maps import NoiseMaps
    from tests.projector_mask_models import proj_mask
    G, _ = models()
    imgs, wp = rows_inputs(3)[:2].contiguous(), start_wp(2)
    mask = proj_mask().cuda()
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        def two(st, mask_):
            st.begin_image(imgs, wp, mask=mask_)
            st.step(imgs)
            r = st.step(imgs)
            return r["styles"].clone(), r["dist"].clone(), r
        s_m, d_m, r_m = two(make_stage(), mask)
        s_p, d_p, r_p = two(make_stage(), None)
        assert "mask_cover" in r_m and "mask_cover" not in r_p
        assert np.abs(r_m["mask_cover"].cpu().numpy() - mask.mean(dim=(1, 2, 3)).cpu().numpy()).max() < 1e-6
        assert not torch.equal(s_m, s_p) and not torch.equal(d_m, d_p)
        st = make_stage()
        st.begin_image(imgs, wp, mask=mask)
        st.capture(imgs, warmup=1)
        r = st.replay()
        torch.cuda.synchronize()
        assert torch.equal(r["styles"], s_m) and torch.equal(r["dist"], d_m)
        with pytest.raises(ValueError, match="captured with a mask"):
            st.begin_image(imgs, wp)
        # shared maps: the stage goes on with the maps it is given
        shared = NoiseMaps(G.synthesis, 2, imgs.device)
        shared.reset()
        with torch.no_grad():
            shared.maps[8].mul_(-1.0)
        before = shared.flat.detach().clone()
        st2 = make_stage()
        st2.begin_image(imgs, wp, noises=shared)
        assert st2.noise is shared and torch.equal(shared.flat.detach(), before)
        st2.step(imgs)
        st2.step(imgs)
        assert not torch.equal(shared.flat.detach(), before)
        with pytest.raises(ValueError, match="pass it again"):
            st2.begin_image(imgs, wp)
    finally:
        ops.set_deterministic(was)


def test_cli_run_with_s_steps_writes_codes_that_reproduce_the_image(tmp_path):
    """main() with --steps 2 --s_steps 3 --batch_size 2 on a [3,3,64,64] .pt (a captured first group, a padded second group on the
    same two graphs): id{n}-s.pt and id{n}-noise.pt reloaded into synthesis(styles=..., noises=...) give rec/{n:05d}.png byte for
    byte; id{n}-wp.pt stays the W result (its image differs); Loss.txt holds the S stage's lines behind the W stage's."""
    import os
    from PIL import Image
    from dge_amd import ops
    from dge_amd.infer import quantize_u8
    from dge_amd.projector import main
    from dge_amd.style_codes import StyleCodes
    N = 3
    imgs = torch.rand(N, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    torch.save(imgs, tmp_path / "imgs.pt")
    out = tmp_path / "out"
    was = ops.is_deterministic()
    try:
        st = main(["--steps", "2", "--s_steps", "3", "--s_lr", "0.02", "--batch_size", "2", "--allow_standin_lpips", "--img_size", "64",
                   "--fmaps_base", "2048", "--fmaps_max", "128", "--compute_dtype", "f32", "--w_avg_samples", "64", "--save_every", "1",
                   "--img_dir", str(tmp_path / "imgs.pt"), "--experiment_dir", str(out), "--deterministic", "true"])
        sst = st.style_stage
        assert sst.captured and sst.it == 3 and sst.group == 1 and sst.lr == 0.02 and sst.noise is st.noise
        for n in range(N):
            rows, maps, wp = (torch.load(out / "models" / f"id{n}-{k}.pt") for k in ("s", "noise", "wp"))
            assert [tuple(x.shape) for x in rows] == [(1, C) for C in sst.codes.channels]
            codes = StyleCodes(st.G.synthesis, 1, "cuda")
            codes.load_rows(0, [x.cuda() for x in rows])
            with torch.no_grad():
                img = st.G.synthesis(styles=codes, noises=[x.cuda() for x in maps])["image"]
                img_w = st.G.synthesis(wp.cuda(), noises=[x.cuda() for x in maps])["image"]
            rec = np.asarray(Image.open(out / "rec" / f"{n:05d}.png"))
            assert np.array_equal(rec, quantize_u8(img)[0].cpu().numpy())
            assert not torch.equal(img, img_w)
        lines = open(out / "Loss.txt").read().splitlines()
        want = []
        for group in ((0, 1), (2,)):
            want += [f"id_{n}_____i_{i}" for i in range(2) for n in group] + [f"id_{n}_____s_{i}" for i in range(3) for n in group]
        assert [ln.split()[0] for ln in lines] == want
        assert sorted(os.listdir(out / "models")) == sorted(f"id{n}-{k}.pt" for n in range(N) for k in ("w", "wp", "noise", "s"))
    finally:
        ops.set_deterministic(was)
