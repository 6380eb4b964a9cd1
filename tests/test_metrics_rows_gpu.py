"""dge_image_metrics_u8 / dge_quantize_u8 on the device against the integer restatement of tests/test_metrics_rows.py.

Bounds: the integer sums are exact.  mse, cosine and a finite psnr are a handful of float64 operations on those integers (one
division; a square root, a product and a division; a division and a log10): 1e-12 relative covers them a thousand times over.
The SSIM mean uses the same integers as the restatement; only the f64 division, contraction and the summation order over at most
65 * 129 = 8 385 windows per channel differ: 1e-12 absolute on values of magnitude <= 1."""
import numpy as np
import pytest
import torch

from tests.test_metrics_rows import expected, pairs

pytestmark = pytest.mark.gpu

SHAPES = [(7, 7), (8, 23), (23, 39), (71, 135)]      # one window; ragged, narrower than a tile; 65 x 129 windows: one past 16/32/64/128
NAMES = ("noisy", "inverted", "identical", "black_white", "flat")


def _dev(arrs):
    return torch.from_numpy(np.stack(arrs)).cuda()


def _check_row(size, name, m, i):
    s, psnr, ssim, mse, cos = expected(*size, name)
    tag = (size, name, i)
    assert m["isums"][i].tolist() == s, tag
    got = {k: float(m[k][i]) for k in ("psnr", "ssim", "mse", "cosine")}
    print("METRICS", tag, got, "ssim err %.2e" % abs(got["ssim"] - ssim))
    assert abs(got["mse"] - mse) <= 1e-12 * abs(mse), tag
    assert abs(got["cosine"] - cos) <= 1e-12 * abs(cos), tag
    if mse == 0:
        assert got["psnr"] == float("inf") and got["ssim"] == 1.0, tag
    else:
        assert abs(got["psnr"] - psnr) <= 1e-12 * abs(psnr), tag
    assert abs(got["ssim"] - ssim) < 1e-12, tag


@pytest.mark.parametrize("size", SHAPES)
def test_image_metrics_rows_match_the_integer_restatement(size):
    from dge_amd.infer import image_metrics_rows
    p = pairs(*size)
    single = {}
    for name in NAMES:
        m = image_metrics_rows(_dev([p[name][0]]), _dev([p[name][1]]))
        assert all(m[k].dtype == torch.float64 and tuple(m[k].shape) == (1,) for k in ("psnr", "ssim", "mse", "cosine"))
        assert m["isums"].dtype == torch.int64 and tuple(m["isums"].shape) == (1, 5)
        _check_row(size, name, m, 0)
        single[name] = m
    # B = 3, three different pairs: every row carries the bits of that pair's B = 1 result
    for trio in (("noisy", "inverted", "flat"), ("identical", "black_white", "noisy")):
        m3 = image_metrics_rows(_dev([p[n][0] for n in trio]), _dev([p[n][1] for n in trio]))
        for i, name in enumerate(trio):
            _check_row(size, name, m3, i)
            for k in ("psnr", "ssim", "mse", "cosine", "isums"):
                assert torch.equal(m3[k][i], single[name][k][0]), (size, trio, i, k)


@pytest.mark.parametrize("size", [(8, 23), (71, 135)])
def test_image_metrics_u8_needs_no_zeroed_buffers_and_is_bit_stable_in_both_modes(size):
    from dge_amd import ops
    p = pairs(*size)
    trio = ("noisy", "inverted", "flat")
    a, b = _dev([p[n][0] for n in trio]), _dev([p[n][1] for n in trio])
    nbytes = ops.image_metrics_u8_work_bytes(3, *size)
    assert nbytes > 0 and nbytes % 8 == 0
    was = ops.is_deterministic()
    results = []
    try:
        for det in (False, True, False):
            ops.set_deterministic(det)
            for _ in range(2):
                bufs = [torch.full((nbytes // 8,), -1, dtype=torch.int64, device="cuda"),                  # 0xFF bytes everywhere
                        torch.full((3, 5), -1, dtype=torch.int64, device="cuda"),
                        torch.full((3,), -1, dtype=torch.int64, device="cuda").view(torch.float64),
                        torch.full((3, 4), -1, dtype=torch.int64, device="cuda").view(torch.float64)]
                isums, ssim, out = ops.image_metrics_u8(a, b, *bufs)
                results.append([t.clone().view(torch.int64) for t in (isums, ssim, out)] + [bufs[0].clone()])
    finally:
        ops.set_deterministic(was)
    for r in results[1:]:
        for x, y in zip(results[0], r):
            assert torch.equal(x, y)
    assert not bool((results[0][3] == -1).any())                                         # every slot of `work` was written
    assert torch.isfinite(results[0][2].view(torch.float64)).all()
    for i, name in enumerate(trio):
        assert results[0][0][i].tolist() == expected(*size, name)[0]


def test_kernel_log_names_the_new_launches_only():
    from dge_amd import ops
    from dge_amd.infer import image_metrics_rows
    p = pairs(23, 39)
    x = torch.from_numpy(p["noisy"][0].copy()).cuda().permute(2, 0, 1).float().div(255).mul(2).sub(1).unsqueeze(0).contiguous()
    ops.KERNEL_LOG = []
    try:
        image_metrics_rows(x, _dev([p["noisy"][1]]))
        names = [n for n, _ in ops.KERNEL_LOG]
    finally:
        ops.KERNEL_LOG = None
    assert names == ["quantize_u8<f32>", "image_metrics_u8"], names
    assert not any("ssim_box7" in n or "loss_reduce" in n for n in names)


def _quantize_inputs(shape):
    """a grid through [-1.01, 1.01] and, for every byte boundary k + 0.5, the f32 next to (k + 0.5)/127.5 - 1 and its two neighbours"""
    n = int(np.prod(shape))
    k = np.arange(255, dtype=np.float64)
    mid = ((k + 0.5) / 127.5 - 1.0).astype(np.float32)
    edge = np.concatenate([np.nextafter(mid, np.float32(-2)), mid, np.nextafter(mid, np.float32(2)),
                           np.array([-1.0, 1.0, 0.0, -0.0, -1.01, 1.01, -3.0, 3.0, 1e-30, -1e-30], dtype=np.float32)])
    if edge.size > n // 2:
        edge = edge[:: -(-edge.size // (n // 2))]                        # the small shape takes an even subset of the boundaries
    grid = np.linspace(-1.01, 1.01, n - edge.size, dtype=np.float64).astype(np.float32)
    v = np.concatenate([edge, grid])
    np.random.default_rng(5).shuffle(v)
    return torch.from_numpy(v.reshape(shape))


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 3, 64, 48)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_u8_equals_the_host_formula(shape, dtype):
    from dge_amd.infer import quantize_u8
    x = _quantize_inputs(shape).to(dtype)
    want = ((x.float() * 0.5 + 0.5).clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    got = quantize_u8(x.cuda())
    assert got.dtype == torch.uint8 and tuple(got.shape) == (shape[0], shape[2], shape[3], shape[1]) and got.is_contiguous()
    assert torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    if shape[3] == 48 and dtype == torch.float32:
        assert int(want.min()) == 0 and int(want.max()) == 255 and len(torch.unique(want)) == 256


def test_image_metrics_rows_on_floats_are_the_metrics_of_their_bytes():
    from dge_amd.infer import image_metrics_rows, quantize_u8
    g = torch.Generator().manual_seed(3)
    a = (torch.rand((2, 3, 23, 39), generator=g) * 2.2 - 1.1).cuda()
    b = (a + 0.1 * torch.randn((2, 3, 23, 39), generator=g).cuda()).to(torch.bfloat16)
    m, mq = image_metrics_rows(a, b), image_metrics_rows(quantize_u8(a), quantize_u8(b))
    mixed = image_metrics_rows(a, quantize_u8(b))
    for k in ("psnr", "ssim", "mse", "cosine", "isums"):
        assert torch.equal(m[k], mq[k]) and torch.equal(m[k], mixed[k]), k
    assert "lpips" not in m


def test_refusals():
    from dge_amd import ops
    from dge_amd._lib import DgeError
    from dge_amd.infer import image_metrics_rows
    err = (DgeError, ValueError)
    small = torch.zeros((1, 6, 9, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(err):
        image_metrics_rows(small, small)
    with pytest.raises(err):
        ops.image_metrics_u8(small, small)                                               # the launch itself refuses too
    with pytest.raises(err):
        ops.image_metrics_u8_work_bytes(1, 9, 6)
    ok = torch.zeros((1, 9, 12, 3), dtype=torch.uint8, device="cuda")
    wide = torch.zeros((1, 9, 12, 6), dtype=torch.uint8, device="cuda")[..., ::2]        # non-contiguous [1,9,12,3]
    with pytest.raises(err):
        image_metrics_rows(wide, ok)
    with pytest.raises(err):
        image_metrics_rows(ok.int(), ok.int())                                           # wrong dtype
    with pytest.raises(err):
        image_metrics_rows(torch.zeros((1, 3, 9, 12), dtype=torch.float64, device="cuda"), ok)
    with pytest.raises(err):
        image_metrics_rows(torch.zeros((1, 3, 9, 12), device="cuda"), ok, quantize=False)
    with pytest.raises(err):
        image_metrics_rows(ok, torch.zeros((1, 9, 13, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(err):
        ops.image_metrics_u8(ok, ok, work=torch.empty(1, dtype=torch.int64, device="cuda"))
