"""The per-image evaluation metrics on 8-bit images (comparing-baseline.py:21-45): an integer-sum numpy restatement - the arithmetic
the device launch dge_image_metrics_u8 uses - against the scipy-based skimage restatement of oracle/metrics_ref.py, and the
argument / pairing behaviour of `python -m dge_amd.compare` that needs no GPU.

Every sum over two uint8 images is an integer: the five 7x7 window sums fit int32, the pixel sums int64.  With Sx, Sy, Sxx, Syy,
Sxy the window sums, ux = Sx/49 and vx = (49/48)(Sxx/49 - ux^2) = (49 Sxx - Sx^2)/(48*49), so the SSIM map is
    ((2 Sx Sy + 49^2 C1)(2 (49 Sxy - Sx Sy) + 48*49 C2)) / ((Sx^2 + Sy^2 + 49^2 C1)((49 Sxx - Sx^2) + (49 Syy - Sy^2) + 48*49 C2))
with integer terms: nothing cancels in floating point.  Against the oracle the difference is the float64 rounding of
scipy's uniform_filter (measured 7.5e-14 at worst on the cases below); the bound is 1e-12."""
import functools

import numpy as np
import pytest

C1 = (0.01 * 255.0) * (0.01 * 255.0)
C2 = (0.03 * 255.0) * (0.03 * 255.0)


def box7(x):
    """x int64 [H,W,C] -> [H-6,W-6,C]: the 7x7 window sums by a cumulative-sum table"""
    H, W, Cc = x.shape
    c = np.zeros((H + 1, W + 1, Cc), dtype=np.int64)
    c[1:, 1:] = x.cumsum(0).cumsum(1)
    return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]


def ssim_int(a, b):
    """mean skimage SSIM of two uint8 [H,W,C] images from integer window sums, float64"""
    a, b = a.astype(np.int64), b.astype(np.int64)
    sx, sy, sxx, syy, sxy = box7(a), box7(b), box7(a * a), box7(b * b), box7(a * b)
    k1, k2 = C1 * 2401.0, C2 * 2352.0
    A1 = (2 * sx * sy).astype(np.float64) + k1
    B1 = (sx * sx + sy * sy).astype(np.float64) + k1
    A2 = (2 * (49 * sxy - sx * sy)).astype(np.float64) + k2
    B2 = ((49 * sxx - sx * sx) + (49 * syy - sy * sy)).astype(np.float64) + k2
    S = (A1 * A2) / (B1 * B2)
    return float(S.sum() / S.size)


def int_sums(a, b):
    a, b = a.astype(np.int64).ravel(), b.astype(np.int64).ravel()
    return [int(a.sum()), int(b.sum()), int((a * a).sum()), int((b * b).sum()), int((a * b).sum())]


def metrics_from_sums(s, n):
    """(psnr, mse, cosine) in float64 from the five integer sums of an image pair of n bytes (Python integers: exact)"""
    sa, sb, saa, sbb, sab = s
    sq = saa - 2 * sab + sbb
    mse = float(sq) / float(n)
    psnr = float("inf") if sq == 0 else 10.0 * np.log10(65025.0 / mse)
    num = 4 * sab - 510 * (sa + sb) + 65025 * n
    da, db = 4 * saa - 1020 * sa + 65025 * n, 4 * sbb - 1020 * sb + 65025 * n
    return psnr, mse, float(num) / float(np.sqrt(float(da) * float(db)))


@functools.lru_cache(maxsize=None)
def pairs(H, W):
    """the input pairs of the metric tests at one size: name -> (a, b) uint8 [H,W,3] (computed once, never written to)"""
    rng = np.random.default_rng(1000 * H + W)
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    noisy = np.clip(a.astype(np.int64) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    out = dict(noisy=(a, noisy), inverted=(a, 255 - a), identical=(a, a.copy()),
               black_white=(np.zeros_like(a), np.full_like(a, 255)), flat=(np.full_like(a, 100), np.full_like(a, 120)))
    for x, y in out.values():
        x.setflags(write=False)
        y.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(H, W, name):
    """(isums, psnr, ssim, mse, cosine) of a pair from the restatement above"""
    a, b = pairs(H, W)[name]
    s = int_sums(a, b)
    psnr, mse, cos = metrics_from_sums(s, a.size)
    return s, psnr, ssim_int(a, b), mse, cos


@pytest.mark.parametrize("size", [(7, 7), (8, 23), (23, 39), (70, 65)])
def test_integer_ssim_restatement_matches_the_scipy_restatement(size):
    from oracle.metrics_ref import skimage_ssim
    for name, (a, b) in pairs(*size).items():
        got, ref = ssim_int(a, b), skimage_ssim(a, b)
        assert abs(got - ref) < 1e-12, (size, name, got, ref)


def test_integer_ssim_known_answers():
    for size in ((7, 7), (23, 39)):
        p = pairs(*size)
        assert ssim_int(*p["identical"]) == 1.0                                          # exactly: numerator == denominator in integers
        assert abs(ssim_int(*p["flat"]) - (2 * 100 * 120 + C1) / (100 ** 2 + 120 ** 2 + C1)) < 1e-14
        assert ssim_int(*p["noisy"]) == ssim_int(*p["noisy"][::-1])                      # symmetric to the bit


def test_integer_metrics_match_the_script_formulas():
    """comparing-baseline.py:21-45 in float64 on the 8-bit values: mean squared error, skimage's PSNR, cosine of x/255*2-1"""
    for name, (a, b) in pairs(23, 39).items():
        _, psnr, _, mse, cos = expected(23, 39, name)
        x, y = a.astype(np.float64), b.astype(np.float64)
        m = ((x - y) ** 2).mean()
        assert abs(mse - m) <= 1e-12 * m
        if m > 0:
            assert abs(psnr - 10 * np.log10(255.0 ** 2 / m)) < 1e-11
        else:
            assert psnr == float("inf")
        u, v = (x / 255 * 2 - 1).ravel(), (y / 255 * 2 - 1).ravel()
        assert abs(cos - u @ v / (np.linalg.norm(u) * np.linalg.norm(v))) < 1e-12


# ------------------------------------------------------------------ python -m dge_amd.compare: what runs before the first launch
def _write(folder, name, arr):
    from PIL import Image
    folder.mkdir(exist_ok=True)
    Image.fromarray(arr).save(folder / name)


def test_compare_pairs_files_in_sorted_name_order(tmp_path):
    from dge_amd import compare
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    for n in ("b.png", "a.jpg", "c.PNG", "notes.txt"):
        if n.endswith(".txt"):
            (tmp_path / "x").mkdir(exist_ok=True)
            (tmp_path / "x" / n).write_text("not an image")
        else:
            _write(tmp_path / "x", n, img)
    for n in ("2.png", "10.png", "1.png"):
        _write(tmp_path / "y", n, img)
    assert compare.pair_names(str(tmp_path / "x"), str(tmp_path / "y")) == [("a.jpg", "1.png"), ("b.png", "10.png"), ("c.PNG", "2.png")]
    assert compare.groups([(np.zeros((8, 8, 3)),)] * 3 + [(np.zeros((9, 8, 3)),)] * 2, 2) == [(0, 2), (2, 3), (3, 5)]


def test_compare_refuses_unequal_counts_and_sizes(tmp_path, capsys):
    from dge_amd import compare
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    for n in ("0.png", "1.png"):
        _write(tmp_path / "x", n, img)
    _write(tmp_path / "y", "0.png", img)
    with pytest.raises(SystemExit) as e:
        compare.main(["--dir1", str(tmp_path / "x"), "--dir2", str(tmp_path / "y"), "--out", str(tmp_path / "o")])
    assert "2 images" in str(e.value.code) and "1 in" in str(e.value.code)
    _write(tmp_path / "y", "1.png", np.zeros((8, 9, 3), dtype=np.uint8))
    with pytest.raises(SystemExit) as e:
        compare.main(["--dir1", str(tmp_path / "x"), "--dir2", str(tmp_path / "y"), "--out", str(tmp_path / "o")])
    assert "--img_size" in str(e.value.code) and not (tmp_path / "o").exists()
    (tmp_path / "empty").mkdir()
    with pytest.raises(SystemExit):
        compare.main(["--dir1", str(tmp_path / "empty"), "--dir2", str(tmp_path / "empty")])
    with pytest.raises(SystemExit):
        compare.main(["--dir1", str(tmp_path / "x")])                                    # --dir2 is required
