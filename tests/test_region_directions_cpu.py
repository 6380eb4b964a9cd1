"""The parts of the region directions that need no GPU: the conditions the fixture tests/golden/region.npz was written under, the
numpy float64 restatement of the solve (tests/region_ref.py) against the fixture, the command line's parsing and refusals, and the
module's place below the training scripts."""
import subprocess
import sys

import numpy as np
import pytest

from tests import region_ref as RR
from tests.conftest import ROOT
from tests.region_models import (REGION_GAP, REGION_K, REGION_POOL, REGION_REG, REGION_ROWS, REGION_STEP, fixture, region_basis, region_masks)


def test_fixture_conditions():
    fx = fixture()
    Q = fx["Q"].astype(np.float64)
    assert Q.shape == (REGION_K, 512) and np.abs(Q @ Q.T - np.eye(REGION_K)).max() < 1e-6
    assert np.array_equal(fx["Q"], region_basis().numpy()) and np.array_equal(fx["masks"], region_masks().numpy())
    assert fx["wp"].shape == (1, 10, 512) and fx["X"].shape == (REGION_K, 3 * 32 * 32) and fx["X"].dtype == np.float64
    assert float(fx["step"]) == REGION_STEP and int(fx["pool"]) == REGION_POOL and float(fx["reg"]) == REGION_REG
    assert tuple(fx["rows"]) == REGION_ROWS
    assert set(np.unique(fx["m0_mu"])) == {0.0, 1.0}                                  # even bounds
    assert set(np.unique(fx["m1_mu"])) == {0.0, 0.25, 0.5, 1.0}                       # odd bounds: edges 0.5, corners 0.25
    for i in range(2):
        assert int((fx[f"m{i}_gaps"] >= REGION_GAP).sum()) >= 3
        assert np.array_equal(fx[f"m{i}_gaps"], RR.rel_gaps(fx[f"m{i}_ratio"]))
        e_ref, lam_err = fx[f"m{i}_e_ref"], float(fx[f"m{i}_lam_err_ref"])
        assert e_ref.shape == (2,) and np.all(e_ref > 0) and np.all(e_ref < 1e-3) and 0 < lam_err < 1e-3
        # the reference's f32 Grams reproduce the recorded error
        for k, tag in enumerate(("M_f", "M_b")):
            M = fx[f"m{i}_{tag}"]
            assert np.abs(fx[f"m{i}_{tag}32"] - M).max() / np.abs(M).max() == e_ref[k]


@pytest.mark.parametrize("i", [0, 1])
def test_fixture_grams_and_truncation(i):
    """The float64 Grams are those of the stored operand under the pooled mask, and the finite-difference Grams stand within the
    recorded truncation of the Grams of the exact autograd Jacobian (about 1 % at h = 0.25: documentation, not a bound of a kernel)."""
    fx = fixture()
    mu = RR.pooled_weights(fx["masks"][i, 0], REGION_POOL)
    assert np.array_equal(mu, fx[f"m{i}_mu"])
    M_f, M_b = RR.grams_ref(fx["X"], mu)
    assert np.array_equal(M_f, fx[f"m{i}_M_f"]) or np.abs(M_f - fx[f"m{i}_M_f"]).max() <= 1e-13 * np.abs(M_f).max()
    assert np.abs(M_b - fx[f"m{i}_M_b"]).max() <= 1e-13 * np.abs(M_b).max()
    for k, tag in enumerate(("f", "b")):
        J, M = fx[f"m{i}_J_{tag}"], fx[f"m{i}_M_{tag}"]
        trunc = np.abs(M - J).max() / np.abs(J).max()
        assert trunc == pytest.approx(float(fx[f"m{i}_truncation"][k]), rel=1e-9) and 0 < trunc < 0.05


@pytest.mark.parametrize("i", [0, 1])
def test_solve_restatement_reproduces_the_fixture(i):
    fx = fixture()
    M_f, M_b, Q = fx[f"m{i}_M_f"], fx[f"m{i}_M_b"], fx["Q"]
    eps, lam, c, d = RR.solve_ref(M_f, M_b, REGION_REG, Q)
    assert eps == pytest.approx(float(fx[f"m{i}_eps"]), rel=1e-12) and eps == pytest.approx(REGION_REG * np.trace(M_b) / REGION_K, rel=1e-12)
    assert np.abs(lam - fx[f"m{i}_ratio"]).max() <= 1e-10 * lam[0]
    keep = fx[f"m{i}_gaps"] >= REGION_GAP
    assert np.all(RR.sin_angle(c[keep], fx[f"m{i}_coeffs"][keep]) <= 1e-7)
    assert np.all(RR.sin_angle(d[keep], fx[f"m{i}_directions"][keep]) <= 1e-7)
    # what the solve promises, in float64: descending ratios, unit vectors, the Rayleigh quotient of c_k is ratio_k, and no vector beats ratio_0
    assert np.all(np.diff(lam) <= 0) and np.abs(np.linalg.norm(c, axis=1) - 1).max() < 1e-12
    assert np.abs(RR.rayleigh(c, M_f, M_b, eps) - lam).max() <= 1e-9 * lam[0]
    u = np.random.default_rng(5).standard_normal((64, REGION_K))
    assert np.all(RR.rayleigh(u, M_f, M_b, eps) <= lam[0] * (1 + 1e-9))
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-12
    top = np.argmax(np.abs(d), axis=1)
    assert np.all(d[np.arange(REGION_K), top] > 0)
    # the white mask's limit: tr(M_b) = 0 falls back to tr(M_f), and both zero is refused
    eps_w, lam_w, c_w, _ = RR.solve_ref(M_f + M_b, np.zeros_like(M_b), REGION_REG)
    assert eps_w == pytest.approx(REGION_REG * np.trace(M_f + M_b) / REGION_K)
    ev = np.linalg.eigvalsh(M_f + M_b)[::-1]
    assert np.abs(lam_w * eps_w - ev).max() <= 1e-9 * ev[0]
    with pytest.raises(ValueError):
        RR.region_eps(np.zeros((3, 3)), np.zeros((3, 3)), 1e-3)


BASE = ["fit", "--wp", "a.pt", "--mask_dir", "m.pt", "--out", "o.pt", "--img_size", "64"]


def test_cli_parsing():
    from dge_amd.region_directions import parse_args
    a = parse_args(BASE)
    assert a.compute_dtype == "f32" and a.step == 0.25 and a.reg == 1e-3 and a.batch == 8 and a.jac_res is None and a.row_range is None
    assert a.num_layers == 10 and a.wp == ["a.pt"] and a.noise is None
    a = parse_args(BASE + ["--compute_dtype", "bf16", "--rows", "2-5", "--jac_res", "16", "--wp", "a.pt", "b.pt", "--noise", "x.pt", "y.pt"])
    assert a.compute_dtype == "bf16" and a.row_range == (2, 5) and a.jac_res == 16 and a.wp == ["a.pt", "b.pt"]
    c = parse_args(["check", "--directions", "r.pt", "--wp", "a.pt", "--mask_dir", "m.pt", "--amounts", "0.5,2", "--img_size", "64"])
    assert c.amount_list == [0.5, 2.0]


@pytest.mark.parametrize("extra,message", [
    (["--mtype", "1"], "--mtype must be 2"),
    (["--noise", "x.pt", "y.pt"], "--noise names 2 files, --wp 1"),
    (["--jac_res", "48"], "no power-of-two divisor"),
    (["--jac_res", "128"], "no power-of-two divisor"),
    (["--rows", "3-10"], "outside the 10 rows"),
    (["--step", "0"], "--step 0.0 must be positive"),
    (["--reg", "-1"], "--reg -1.0 must be positive"),
    (["--batch", "3"], "--batch 3 must be even"),
    (["--basis", "b.pt", "--basis_num", "1025"], "K > 1024"),
    (["--basis_num", "4"], "belongs to --basis"),
    (["--num", "0"], "--num must be positive"),
    (["--img_size", "48"], "no power of two"),
])
def test_cli_refusals(extra, message):
    from dge_amd.region_directions import parse_args
    with pytest.raises(SystemExit, match=message):
        parse_args(BASE + extra)


def test_cli_refusals_of_missing_arguments(monkeypatch):
    from dge_amd.region_directions import parse_args
    with pytest.raises(SystemExit, match="--wp and --mask_dir are required"):
        parse_args(["fit", "--out", "o.pt", "--img_size", "64"])
    with pytest.raises(SystemExit, match="--out is required"):
        parse_args(BASE[:5] + ["--img_size", "64"])
    with pytest.raises(SystemExit, match="check needs --directions"):
        parse_args(["check", "--wp", "a.pt", "--mask_dir", "m.pt", "--img_size", "64"])
    with pytest.raises(SystemExit, match="must be positive"):
        parse_args(["check", "--directions", "r.pt", "--wp", "a.pt", "--mask_dir", "m.pt", "--amounts", "0,1", "--img_size", "64"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        parse_args(BASE)


def test_argument_checks_without_a_device():
    from dge_amd.region_directions import _pool_factor, _row_range
    assert _pool_factor(1024, None) == (4, 256) and _pool_factor(64, None) == (1, 64) and _pool_factor(64, 32) == (2, 32)
    for H, r in ((64, 48), (64, 128), (64, 0), (64, 24)):
        with pytest.raises(ValueError, match="power-of-two divisor"):
            _pool_factor(H, r)
    assert _row_range(None, 10) == (0, 10) and _row_range(range(2, 6), 10) == (2, 6) and _row_range([4], 10) == (4, 5)
    with pytest.raises(ValueError, match="outside the 10 rows"):
        _row_range([3, 10], 10)
    with pytest.raises(ValueError, match="consecutive"):
        _row_range([1, 3], 10)


def test_the_module_stays_below_the_training_script():
    code = ("import sys, dge_amd\nimport dge_amd.region_directions\n"
            "assert 'dge_amd.e_align' not in sys.modules, sorted(m for m in sys.modules if m.startswith('dge_amd'))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(ROOT + "/deep-gan-encoders_amd/region_directions.py") as f:
        src = f.read()
    assert "from .e_align" not in src and "import e_align" not in src


def test_chunk_and_workspace_sizes():
    """Host-side size functions of dge_gram_cols: the chunk is 4096 columns up to N = 2^20 and N / 256 in whole 32-column stages
    beyond; the workspace holds two partial 64 x 64 tiles per chunk and upper-triangle tile."""
    from dge_amd import ops
    lib = ops.lib()
    assert ops.gram_cols_chunk(1) == ops.gram_cols_chunk(1 << 20) == 4096
    N = 3 * 1024 * 1024
    assert ops.gram_cols_chunk(N) == 12288 and -(-N // 12288) == 256
    assert lib.dge_gram_cols_work_bytes(512, N) == 2 * 4 * 256 * 36 * 4096
    assert lib.dge_gram_cols_work_bytes(1, 1) == 2 * 4 * 4096
    assert lib.dge_gram_cols_work_bytes(1025, 1) == -1 and lib.dge_gram_cols_chunk(1 << 31) == -1
