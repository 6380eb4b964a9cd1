"""dge_amd.region_directions on the GPU, on the 64^2 generator of tests/region_models.py: the Jacobian Grams against the float64
run of the reference's generator (tests/golden/region.npz) within 4 x the reference's own f32 error, the generalised solve against
its float64 restatement (tests/region_ref.py), the exact properties of the solve, edit_leakage, and the command line end to end."""
import numpy as np
import pytest
import torch

from tests import region_ref as RR
from tests.conftest import meas
from tests.directions_ref import U, eig_tolerance, eigh_ref
from tests.region_models import (REGION_GAP, REGION_JAC_RES, REGION_K, REGION_KW, REGION_REG, REGION_ROWS, REGION_STEP, fixture,
                                 region_state_dict)

pytestmark = pytest.mark.gpu

ROWS = range(*REGION_ROWS)
CLI_MODEL = ["--img_size", "64", "--fmaps_base", "2048", "--fmaps_max", "128"]          # (--compute_dtype: f32 is the default here)


def tiles(path, n, S=64):
    """the n tiles of a one-row save_image_grid PNG (2 px padding) as uint8 [S,S,3]"""
    from PIL import Image
    img = np.asarray(Image.open(path).convert("RGB"))
    assert img.shape == (S + 4, n * (S + 2) + 2, 3)
    return [img[2:2 + S, 2 + i * (S + 2):2 + i * (S + 2) + S] for i in range(n)]


@pytest.fixture(scope="module")
def G():
    import dge_amd
    g = dge_amd.StyleGAN2Generator(64, compute_dtype="f32", **REGION_KW).cuda()
    g.load_state_dict(region_state_dict())
    g.eval()
    return g


@pytest.fixture(scope="module")
def inputs():
    fx = fixture()
    return torch.from_numpy(fx["wp"].copy()).cuda(), torch.from_numpy(fx["Q"].copy()).cuda(), torch.from_numpy(fx["masks"].copy()).cuda()


@pytest.fixture(scope="module")
def grams(G, inputs):
    """the GPU's (M_f, M_b) of both masks, computed once and shared (never modified)"""
    from dge_amd.region_directions import jacobian_grams
    wp, Q, masks = inputs
    return [jacobian_grams(G, wp, masks[i:i + 1], rows=ROWS, basis=Q, step=REGION_STEP, jac_res=REGION_JAC_RES) for i in range(2)]


@pytest.mark.parametrize("i", [0, 1])
def test_grams_match_reference_run(grams, i):
    """|M - M64| <= 4 e_ref max |M64| per matrix: e_ref is the error of the reference generator's own f32 run against its float64 run,
    the factor 4 covers another summation order in the convolutions and in the Gram."""
    fx = fixture()
    for tag, M, k in (("M_f", grams[i][0], 0), ("M_b", grams[i][1], 1)):
        ref, e_ref = fx[f"m{i}_{tag}"], float(fx[f"m{i}_e_ref"][k])
        got = M.cpu().numpy()
        assert got.shape == (REGION_K, REGION_K) and np.array_equal(got, got.T)
        err = float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())
        meas(f"region.grams.mask{i}.{tag}", err=err, bound=4 * e_ref, e_ref=e_ref)
        assert 0 < e_ref < 1e-3 and err <= 4 * e_ref, (tag, err, e_ref)


def check_solve(tag, i, M_f, M_b):
    """ratio within 4 lam_err_ref of ratio_0; for every k whose relative gap g_k is at least 0.02: sin angle(c_k, c_k^ref) <=
    min(4 e_ref / g_k, 0.05), e_ref the larger of the two matrices' - no such k is left out, and there are at least three"""
    from dge_amd.region_directions import solve_region
    fx = fixture()
    lam_ref, c_ref, gaps = fx[f"m{i}_ratio"], fx[f"m{i}_coeffs"], fx[f"m{i}_gaps"]
    e_ref, lam_err_ref = float(fx[f"m{i}_e_ref"].max()), float(fx[f"m{i}_lam_err_ref"])
    ratio, coeffs = solve_region(M_f, M_b, reg=REGION_REG)
    lam, c = ratio.cpu().numpy().astype(np.float64), coeffs.cpu().numpy().astype(np.float64)
    lam_err = float(np.abs(lam - lam_ref).max() / lam_ref[0])
    keep = np.flatnonzero(gaps >= REGION_GAP)
    assert len(keep) >= 3
    sin = RR.sin_angle(c[keep], c_ref[keep])
    bound = np.minimum(4 * e_ref / gaps[keep], 0.05)
    meas(f"region.solve.{tag}.mask{i}", lam_err=lam_err, lam_bound=4 * lam_err_ref, sin_of_bound=float((sin / bound).max()), sin_max=float(sin.max()),
         bound_min=float(bound.min()), vectors=len(keep))
    assert np.all(np.diff(lam) <= 0)
    assert lam_err <= 4 * lam_err_ref, (lam_err, lam_err_ref)
    assert np.all(sin <= bound), (sin, bound)


@pytest.mark.parametrize("i", [0, 1])
def test_solve_matches_reference_run(grams, i):
    fx = fixture()
    f32 = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    check_solve("fixture_grams", i, f32(fx[f"m{i}_M_f"]), f32(fx[f"m{i}_M_b"]))
    check_solve("gpu_grams", i, *grams[i])


@pytest.mark.parametrize("i", [0, 1])
def test_solve_properties(grams, i):
    """Exact linear algebra on the GPU's own Grams: the tolerance is rounding"""
    from dge_amd.region_directions import region_eps, solve_region
    M_f, M_b = grams[i]
    ratio, coeffs = solve_region(M_f, M_b, reg=REGION_REG)
    eps = region_eps(M_f, M_b, REGION_REG)
    Mf, Mb = M_f.cpu().numpy().astype(np.float64), M_b.cpu().numpy().astype(np.float64)
    assert eps == pytest.approx(RR.region_eps(Mf, Mb, REGION_REG), rel=1e-12)
    lam, c = ratio.cpu().numpy().astype(np.float64), coeffs.cpu().numpy().astype(np.float64)
    assert np.all(np.diff(lam) <= 0)
    assert np.abs(np.linalg.norm(c, axis=1) - 1).max() <= 4 * U
    R_c = RR.rayleigh(c, Mf, Mb, eps)
    meas(f"region.solve.rayleigh.mask{i}", rel=float(np.abs(R_c / lam - 1).max()))
    assert np.all(np.abs(R_c - lam) <= 1e-4 * np.abs(lam))
    u = np.random.default_rng(7 + i).standard_normal((64, REGION_K))
    u = np.concatenate((u / np.linalg.norm(u, axis=1, keepdims=True), np.eye(REGION_K)))
    assert np.all(RR.rayleigh(u, Mf, Mb, eps) <= lam[0] * (1 + 1e-4))


def test_all_white_mask_and_repeated_pairs(G, inputs, grams):
    """An all-white mask: M_b is exactly zero and the directions are dge_eigh_sym(M_f)'s (within tau / gap, the eigenvector bound of
    tests/test_linalg_kernels_gpu.py).  Two identical (code, mask) pairs give the bits of one.  Unit directions, the sign rule."""
    from dge_amd import ops
    from dge_amd.region_directions import jacobian_grams, region_directions
    wp, Q, masks = inputs
    white = torch.ones(1, 1, 64, 64, device="cuda")
    M_f, M_b = jacobian_grams(G, wp, white, rows=ROWS, basis=Q, step=REGION_STEP, jac_res=REGION_JAC_RES)
    assert torch.all(M_b == 0) and float(M_f.abs().max()) > 0
    f0, b0 = grams[0]
    total = (f0.double() + b0.double()).cpu().numpy()                 # mu + (1 - mu) = 1: the two Grams of a mask add up to the white one
    assert np.abs(M_f.cpu().numpy() - total).max() <= 2 * (3 * REGION_JAC_RES ** 2 + 17) * U * np.abs(total).max()          # dge_gram_cols' bound, both sides
    kw = dict(rows=ROWS, basis=Q, step=REGION_STEP, jac_res=REGION_JAC_RES, reg=REGION_REG)
    dirs = region_directions(G, [wp], [white], **kw)
    assert torch.equal(dirs["M_f"], M_f) and torch.all(dirs["M_b"] == 0)
    _, V, _ = ops.eigh_sym(M_f)
    c, Vh = dirs["coeffs"].cpu().numpy().astype(np.float64), V.cpu().numpy().astype(np.float64)
    M32 = M_f.cpu().numpy()
    tau, _ = eig_tolerance(M32)
    lam, _ = eigh_ref(M32)
    gap = np.abs(lam[:, None] - lam[None, :]) + np.diag(np.full(REGION_K, np.inf))
    bound = np.minimum(tau / gap.min(axis=1), 0.05)
    sin = RR.sin_angle(c, Vh)
    meas("region.white.vectors", sin_of_bound=float((sin / bound).max()))
    assert np.all(sin <= bound), (sin, bound)
    # two identical pairs: the mean of two equal Grams is the Gram, and everything behind it has the same bits
    one = region_directions(G, [wp], [masks[1:2]], **kw)
    two = region_directions(G, [wp, wp], [masks[1:2], masks[1:2]], **kw)
    assert one["images"] == 1 and two["images"] == 2
    for k in ("M_f", "M_b", "directions", "ratio", "fg", "bg", "coeffs"):
        assert torch.equal(one[k], two[k]), k
    assert torch.equal(one["M_f"], grams[1][0]) and torch.equal(one["M_b"], grams[1][1])
    # the dict: every key of a directions file, unit directions with their largest component positive, fg / bg of the coefficients
    from dge_amd.directions import KEYS
    assert all(k in one for k in KEYS) and one["method"] == "region" and one["rows"] == list(ROWS) and one["mean"] is None
    assert torch.equal(one["sigma"], torch.ones(REGION_K, device="cuda")) and torch.equal(one["eigenvalues"], one["ratio"])
    assert one["jac_res"] == REGION_JAC_RES and one["step"] == REGION_STEP and one["reg"] == REGION_REG
    d = one["directions"].cpu().numpy().astype(np.float64)
    assert d.shape == (REGION_K, 512) and (np.linalg.norm(d, axis=1) - 1).max() <= 2.4e-7
    top = np.argmax(np.abs(one["directions"].cpu().numpy()), axis=1)
    assert np.all(d[np.arange(REGION_K), top] > 0)
    cc = one["coeffs"].cpu().numpy().astype(np.float64)
    Qh = Q.cpu().numpy().astype(np.float64)
    assert np.abs(cc @ Qh - d).max() <= 1e-6                          # d_k = normalise(c_k Q), the sign carried to c_k
    Mf, Mb = one["M_f"].cpu().numpy().astype(np.float64), one["M_b"].cpu().numpy().astype(np.float64)
    for key, M in (("fg", Mf), ("bg", Mb)):
        want = np.sum((cc @ M) * cc, axis=1)
        assert np.abs(one[key].cpu().numpy() - want).max() <= 1e-5 * np.abs(M).max(), key
    few = region_directions(G, [wp], [masks[1:2]], num=3, **kw)
    assert tuple(few["directions"].shape) == (3, 512) and torch.equal(few["directions"], one["directions"][:3])


def test_edit_leakage(G, inputs):
    """At amount = h along basis axis 0 the measured sums are (2h)^2 M[0,0] of jacobian_grams on the one-axis basis Q[0:1]: the same
    images and the same kernels at K = 1, up to the rounding of the two scales ((2h)^2 = 0.25 and the scales are powers of two
    here: the bound is dge_gram_cols' own, on both sides)."""
    from dge_amd.region_directions import edit_leakage, jacobian_grams
    wp, Q, masks = inputs
    h = REGION_STEP
    dirs = dict(directions=Q[0:1], rows=list(ROWS), jac_res=REGION_JAC_RES)
    for i in range(2):
        M_f, M_b = jacobian_grams(G, wp, masks[i:i + 1], rows=ROWS, basis=Q[0:1], step=h, jac_res=REGION_JAC_RES)
        fg, bg = edit_leakage(G, wp, masks[i:i + 1], dirs, 0, h)
        N = 3 * REGION_JAC_RES ** 2
        tol = 2 * (N + 1 + 16) * U                                    # relative: every term of a diagonal element is positive
        want_f, want_b = (2 * h) ** 2 * float(M_f), (2 * h) ** 2 * float(M_b)
        meas(f"region.leakage.mask{i}", fg_rel=abs(fg / want_f - 1), bg_rel=abs(bg / want_b - 1), tol=tol)
        assert fg > 0 and bg > 0 and abs(fg - want_f) <= tol * want_f and abs(bg - want_b) <= tol * want_b
    with pytest.raises(ValueError, match="outside the 1 directions"):
        edit_leakage(G, wp, masks[:1], dirs, 1, h)


def test_api_refusals(G, inputs):
    from dge_amd.region_directions import jacobian_grams, region_directions, solve_region
    wp, Q, masks = inputs
    m = masks[:1]
    with pytest.raises(ValueError, match="step"):
        jacobian_grams(G, wp, m, basis=Q, step=0.0)
    with pytest.raises(ValueError, match="must be even"):
        jacobian_grams(G, wp, m, basis=Q, batch=3)
    with pytest.raises(ValueError, match="power-of-two divisor"):
        jacobian_grams(G, wp, m, basis=Q, jac_res=48)
    with pytest.raises(ValueError, match="outside the 10 rows"):
        jacobian_grams(G, wp, m, basis=Q, rows=range(3, 11))
    with pytest.raises(ValueError, match="a mask holds"):
        jacobian_grams(G, wp, torch.ones(1, 1, 32, 32), basis=Q)
    with pytest.raises(ValueError, match="not orthonormal"):
        jacobian_grams(G, wp, m, basis=Q * 1.001)
    with pytest.raises(ValueError, match="at most 1024"):
        jacobian_grams(G, wp, m, basis=torch.zeros(1025, 512, device="cuda"))
    with pytest.raises(ValueError, match="one of each per image"):
        region_directions(G, [wp, wp], [m], basis=Q)
    with pytest.raises(ValueError, match="reg"):
        solve_region(torch.eye(3, device="cuda"), torch.eye(3, device="cuda"), reg=0.0)
    with pytest.raises(ValueError, match="trace 0"):
        solve_region(torch.zeros(3, 3, device="cuda"), torch.zeros(3, 3, device="cuda"))


def test_cli_fit_check_apply_and_untouched_synthesis(G, inputs, tmp_path, capsys):
    from dge_amd import directions, ops, region_directions as RD
    from dge_amd.infer import quantize_u8
    wp, Q, masks = inputs
    ckpt = str(tmp_path / "g.pt")
    torch.save({"generator_smooth": region_state_dict()}, ckpt)
    model = CLI_MODEL + ["--checkpoint_dir_GAN", ckpt]
    torch.save(wp.cpu(), tmp_path / "wp.pt")
    torch.save(masks[:1].cpu(), tmp_path / "mask.pt")
    basis = dict(directions=Q.cpu(), eigenvalues=torch.ones(REGION_K), sigma=torch.ones(REGION_K), mean=None, method="sefa", rows=list(ROWS),
                 samples=None, seed=None)
    directions.save_directions(basis, str(tmp_path / "basis.pt"))

    def logged():
        ops.KERNEL_LOG, ops.PROFILE = log, prof = [], []
        try:
            with torch.no_grad():
                img = G.synthesis(wp)["image"].clone()
            return ([(n, s.value) for n, s in log], [e[3] for e in prof]), img
        finally:
            ops.KERNEL_LOG = ops.PROFILE = None
    before, img0 = logged()
    out = str(tmp_path / "region.pt")
    common = ["--wp", str(tmp_path / "wp.pt"), "--mask_dir", str(tmp_path / "mask.pt")] + model
    ops.KERNEL_LOG = []
    try:
        dirs = RD.main(["fit", "--basis", str(tmp_path / "basis.pt"), "--basis_num", "8", "--jac_res", "32", "--num", "4", "--out", out] + common)
        fit_log = [n for n, _ in ops.KERNEL_LOG]
    finally:
        ops.KERNEL_LOG = None
    after, img1 = logged()
    assert before[1] and before == after and torch.equal(img0, img1)          # a plain synthesis issues the launches it issued before
    # 8 axes, 4 per synthesis call: two groups, one Gram, the solve's two eigendecompositions
    assert fit_log.count("wp_axis_pairs") == 2 and fit_log.count("fd_pool_diff") == 2 and fit_log.count("gram_cols") == 1
    assert fit_log.count("eigh_sym") == 2 and fit_log.count("matmul_f64acc") >= 4
    lines = [l for l in capsys.readouterr().out.splitlines() if "ratio" in l]
    assert len(lines) == 4 and lines[0].split()[0] == "0" and "fg" in lines[0] and "bg" in lines[0]
    saved = directions.load_directions(out)
    assert tuple(saved["directions"].shape) == (4, 512) and saved["method"] == "region" and not saved["directions"].is_cuda
    assert torch.equal(saved["directions"], dirs["directions"].cpu()) and torch.equal(saved["ratio"], dirs["ratio"].cpu())
    assert saved["jac_res"] == 32 and saved["images"] == 1 and tuple(saved["coeffs"].shape) == (4, 8)
    directions.save_directions(dirs, str(tmp_path / "plain.pt"))              # the dict passes save_directions unchanged
    assert torch.equal(directions.load_directions(str(tmp_path / "plain.pt"))["directions"], saved["directions"])
    # rendering is `directions apply`, unchanged: amount 0 gives the bytes of the unedited code's image
    strip = str(tmp_path / "strip.png")
    directions.main(["apply", "--directions", out, "--wp", str(tmp_path / "wp.pt"), "--index", "0", "--amounts=0,2", "--out", strip,
                     "--compute_dtype", "f32"] + model)
    t0, t1 = tiles(strip, 2)
    with torch.no_grad():
        q = quantize_u8(G.synthesis(wp)["image"])[0].cpu().numpy()
    assert np.array_equal(t0, q) and not np.array_equal(t1, q)
    # check: edit_leakage per direction and amount
    capsys.readouterr()
    rows = RD.main(["check", "--directions", out, "--amounts", "0.5"] + common)
    printed = [l for l in capsys.readouterr().out.splitlines() if l.startswith("image 0")]
    assert len(rows) == 4 and len(printed) == 4
    fg, bg = RD.edit_leakage(G, wp, masks[:1], saved, 0, 0.5)
    assert rows[0] == (0, 0, 0.5, fg, bg) and fg > 0 and bg > 0
    # refusals that need the files
    torch.save(torch.ones(1, 1, 32, 32), tmp_path / "small.pt")
    torch.save(masks.cpu(), tmp_path / "two.pt")
    torch.save(wp.cpu()[:, :8], tmp_path / "short.pt")
    bad = dict(basis)
    bad["directions"] = Q.cpu() * 1.01
    directions.save_directions(bad, str(tmp_path / "bad_basis.pt"))
    fit = lambda extra, wpf="wp.pt", mask="mask.pt": RD.main(["fit", "--out", out, "--wp", str(tmp_path / wpf), "--mask_dir", str(tmp_path / mask)]
                                                            + extra + model)
    with pytest.raises(SystemExit, match="the masks are"):
        fit([], mask="small.pt")
    with pytest.raises(SystemExit, match="holds 2 masks"):
        fit([], mask="two.pt")
    with pytest.raises(SystemExit, match="holds"):
        fit([], wpf="short.pt")
    with pytest.raises(SystemExit, match="not orthonormal"):
        fit(["--basis", str(tmp_path / "bad_basis.pt")])
    with pytest.raises(SystemExit, match="above the 16 directions"):
        fit(["--basis", str(tmp_path / "basis.pt"), "--basis_num", "17"])
