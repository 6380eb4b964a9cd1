"""The kernels of csrc/region_kernels.hip at the smallest shapes where each can go wrong, against float64 on the same f32 operands
within bounds derived from each kernel's own arithmetic, and the exact properties (symmetry, equal bits from run to run and in both
reduction modes, untouched padding, refusals that write nothing)."""
import numpy as np
import pytest
import torch

from tests import region_ref as RR
from tests.conftest import meas
from tests.golden import recipe as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def both_modes(fn):
    """fn() in the default and in the deterministic reduction mode (twice): the same bits -> the result"""
    from dge_amd import ops
    was = ops.is_deterministic()
    outs = []
    try:
        for on in (False, True, True):
            ops.set_deterministic(on)
            outs.append(fn().clone())
    finally:
        ops.set_deterministic(was)
    for o in outs[1:]:
        assert torch.equal(outs[0], o)
    return outs[0]


# ------------------------------------------------------------------ dge_gram_cols
def _chunk():
    from dge_amd import ops
    return ops.gram_cols_chunk(1)


GRAM_COLS = [(1, 1, 1), (3, 7, 7), (5, 12, 4), (33, 1026, 513), (65, 768, 256), (130, 3072, 1024), (512, 1536, 512)]
AROUND_CHUNK = [(5, -1), (5, 0), (5, 1), (66, 1)]          # (K, N - the chunk): one below, at and one above the column chunk


def gram_cols_case(K, N, P, tag):
    """Per element |out - ref| <= (c + n_c + 16) 2^-24 sum_n |w_n x_in x_jn| (tests/region_ref.py gram_cols_ref): the c columns of a
    chunk are accumulated in one f32 accumulator (a rounding per fma), the n_c chunk sums are added in order (a rounding each), and
    the 16 cover the one rounding of w_n x_jn in the operand, of the scale and of the store.  With the weight, without it, on a
    contiguous operand and on a view with ldx > N; every result symmetric to the bit and the same in a second call and in both
    reduction modes."""
    from dge_amd import ops
    chunk = ops.gram_cols_chunk(N)
    x = R.randn(f"region.gram_cols.{K}x{N}", (K, N + 5), 41)
    if K > 1:
        x[1] = 0.0
    w = torch.rand(P, generator=torch.Generator().manual_seed(N + P))
    w[0] = 0.0
    w[-1] = 1.0
    wide, wd = x.cuda(), w.cuda()
    worst = 0.0
    for view in (False, True):
        xd = wide[:, 3:3 + N] if view else wide[:, 3:3 + N].contiguous()
        assert (xd.stride(0) > N) == view or K == 1
        xh = x[:, 3:3 + N].numpy()
        for wgt, scale in ((wd, 0.37), (None, 1.0)):
            if wgt is None:
                a = both_modes(lambda: ops.gram_cols(xd, scale=scale))
                outs = [a]
                assert torch.equal(ops.gram_cols(xd, scale=scale), a)
            else:
                a = both_modes(lambda: ops.gram_cols(xd, wgt=wgt, scale=scale)[0])
                b = both_modes(lambda: ops.gram_cols(xd, wgt=wgt, scale=scale)[1])
                outs = [a, b]
                a2, b2 = ops.gram_cols(xd, wgt=wgt, scale=scale)
                assert torch.equal(a2, a) and torch.equal(b2, b)
                assert torch.equal(ops.gram_cols(xd, wgt=wgt, scale=scale, both=False), a)          # out_b = NULL: the same out_a
            assert ops.last_kernel() == "gram_cols"
            ra, rb, ba, bb = RR.gram_cols_ref(xh, None if wgt is None else w.numpy(), chunk, float(np.float32(scale)))
            for out, ref, bound in zip(outs, (ra, rb), (ba, bb)):
                assert tuple(out.shape) == (K, K) and torch.equal(out, out.t())
                err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
                assert np.all(err <= bound), (tag, view, wgt is None, float((err - bound).max()))
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    meas(f"region.gram_cols.{tag}", of_bound=worst)


@pytest.mark.parametrize("K,N,P", GRAM_COLS)
def test_gram_cols_against_float64(K, N, P):
    gram_cols_case(K, N, P, f"{K}x{N}")


@pytest.mark.parametrize("K,dn", AROUND_CHUNK)
def test_gram_cols_around_the_chunk(K, dn):
    N = _chunk() + dn
    gram_cols_case(K, N, N if dn else 1024, f"{K}xchunk{dn:+d}")


def test_gram_cols_long_rows_change_the_chunk():
    """Beyond N = 2^20 the chunk grows with N (256 chunks at the most): one case on that path, K = 2"""
    from dge_amd import ops
    N = (1 << 20) + 96
    chunk = ops.gram_cols_chunk(N)
    assert chunk > _chunk() and chunk % 32 == 0 and -(-N // chunk) <= 256
    x = R.randn("region.gram_cols.long", (2, N), 42)
    w = torch.rand(N // 32, generator=torch.Generator().manual_seed(3))
    a, b = ops.gram_cols(x.cuda(), wgt=w.cuda())
    ra, rb, ba, bb = RR.gram_cols_ref(x.numpy(), w.numpy(), chunk)
    assert np.all(np.abs(a.cpu().numpy() - ra) <= ba) and np.all(np.abs(b.cpu().numpy() - rb) <= bb)


def test_gram_cols_exact_weights():
    from dge_amd import ops
    K, N, P = 37, 1100, 275
    x = R.randn("region.gram_cols.exact", (K, N), 43).cuda()
    zero, one = torch.zeros(P, device="cuda"), torch.ones(P, device="cuda")
    a0, b0 = ops.gram_cols(x, wgt=zero)
    a1, b1 = ops.gram_cols(x, wgt=one)
    plain = ops.gram_cols(x)
    assert torch.all(a0 == 0) and torch.all(b1 == 0)                  # w = 0 and 1.0f - 1 = 0: every product is a zero
    assert torch.equal(a1, plain) and torch.equal(b0, plain)          # w = 1: the operand unchanged, the bits of the unweighted kernel
    assert float(plain.abs().min()) > 0


def test_gram_cols_refusals():
    from dge_amd import ops
    from dge_amd._lib import DgeError
    x = torch.ones(4, 8, device="cuda")
    w = torch.full((4,), 0.5, device="cuda")
    for bad, kw in ((torch.ones(1025, 4, device="cuda"), {}), (torch.ones(0, 8, device="cuda"), {}), (torch.ones(4, 0, device="cuda"), {}),
                    (x, dict(wgt=torch.ones(3, device="cuda"))), (x, dict(both=True)), (x, dict(wgt=w.double())), (x, dict(wgt=w.cpu())),
                    (x.double(), {}), (x.t(), {}), (x.cpu(), {}), (torch.ones(8, device="cuda"), {})):
        with pytest.raises(DgeError):
            ops.gram_cols(bad, **kw)
    lib = ops.lib()
    assert lib.dge_gram_cols_work_bytes(0, 8) == -1 and lib.dge_gram_cols_work_bytes(1025, 8) == -1 and lib.dge_gram_cols_work_bytes(4, 0) == -1
    assert lib.dge_gram_cols_work_bytes(4, 1 << 31) == -1 and lib.dge_gram_cols_chunk(0) == -1
    nb = lib.dge_gram_cols_work_bytes(4, 8)
    work = torch.full((nb // 4,), 7.0, device="cuda")
    out_a, out_b = torch.full((4, 4), 7.0, device="cuda"), torch.full((4, 4), 7.0, device="cuda")
    P = lambda t: ops._p(t)
    st = ops._stream()
    assert lib.dge_gram_cols(P(x), 4, 8, 7, P(w), 4, 1.0, P(out_a), P(out_b), P(work), nb, st) == -1          # a row stride below N
    assert lib.dge_gram_cols(P(x), 4, 8, 8, P(w), 3, 1.0, P(out_a), P(out_b), P(work), nb, st) == -1          # P does not divide N
    assert lib.dge_gram_cols(P(x), 4, 8, 8, P(w), 0, 1.0, P(out_a), P(out_b), P(work), nb, st) == -1
    assert lib.dge_gram_cols(P(x), 4, 8, 8, None, 4, 1.0, P(out_a), P(out_b), P(work), nb, st) == -1          # out_b without a weight
    assert lib.dge_gram_cols(P(x), 4, 8, 8, P(w), 4, 1.0, P(out_a), P(out_b), P(work), nb - 4, st) == -1      # a workspace too small
    assert lib.dge_gram_cols(P(x), 4, 8, 8, P(w), 4, 1.0, None, P(out_b), P(work), nb, st) == -1
    assert lib.dge_gram_cols(None, 4, 8, 8, P(w), 4, 1.0, P(out_a), P(out_b), P(work), nb, st) == -1
    assert b"gram_cols" in lib.dge_last_error()
    torch.cuda.synchronize()
    assert torch.all(out_a == 7.0) and torch.all(out_b == 7.0) and torch.all(work == 7.0)          # a refused call touches nothing
    a, b = ops.gram_cols(x, wgt=w)
    assert torch.equal(a, torch.full((4, 4), 4.0, device="cuda")) and torch.equal(b, a)


# ------------------------------------------------------------------ dge_fd_pool_diff
def test_fd_pool_diff_single_pixel_bits():
    """s = 1: the bits of (a - b) * scale with each operation rounded to f32"""
    from dge_amd import ops
    img = R.randn("region.fd.s1", (4, 3, 8, 8), 51)
    scale = float(np.float32(1.0 / (2 * 0.3)))
    x = torch.empty(2, 3 * 64, device="cuda")
    ops.fd_pool_diff(img.cuda(), 1, scale, x)
    assert ops.last_kernel() == "fd_pool_diff"
    a, b = img[0::2].numpy(), img[1::2].numpy()
    want = ((a - b).astype(np.float32) * np.float32(scale)).astype(np.float32).reshape(2, -1)
    assert np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("H", [8, 16])
@pytest.mark.parametrize("n", [1, 3])
def test_fd_pool_diff_against_float64(s, H, n):
    """|x - ref| <= (s^2 + 2) 2^-24 scale sum_window |a - b|: the rounding of each difference, s^2 - 1 additions and the
    multiplication.  The rows of x are a slice of a wider matrix: its padding keeps its bits."""
    from dge_amd import ops
    img = R.randn(f"region.fd.{s}.{H}.{n}", (2 * n, 3, H, H), 52)
    h = 0.25
    scale = float(np.float32(1.0 / (2 * h * s * s)))
    r = H // s
    N = 3 * r * r
    wide = torch.full((n, N + 7), 7.0, device="cuda")
    x = wide[:, 2:2 + N]
    ops.fd_pool_diff(img.cuda(), s, scale, x)
    d = img[0::2].double().numpy() - img[1::2].double().numpy()
    win = lambda t: t.reshape(n, 3, r, s, r, s).transpose(0, 1, 2, 4, 3, 5).reshape(n, 3, r, r, s * s)
    ref = scale * win(d).sum(axis=-1).reshape(n, N)
    bound = (s * s + 2) * U * scale * np.abs(win(d)).sum(axis=-1).reshape(n, N)
    got = wide.cpu().numpy()
    err = np.abs(got[:, 2:2 + N].astype(np.float64) - ref)
    assert np.all(err <= bound), float((err / bound).max())
    assert np.all(got[:, :2] == 7.0) and np.all(got[:, 2 + N:] == 7.0)
    meas(f"region.fd_pool_diff.s{s}.H{H}.n{n}", of_bound=float((err / bound).max()))


def test_fd_pool_diff_refusals():
    from dge_amd import ops
    from dge_amd._lib import DgeError
    img = torch.ones(2, 3, 8, 8, device="cuda")
    x = torch.full((1, 48), 7.0, device="cuda")
    for bad_img, s, bad_x in ((img, 3, x), (img, 2, torch.ones(1, 47, device="cuda")), (img[:1], 2, x), (img, 2, torch.ones(2, 48, device="cuda")),
                              (img, 0, x), (img.double(), 2, x)):
        with pytest.raises(DgeError):
            ops.fd_pool_diff(bad_img, s, 1.0, bad_x)
    torch.cuda.synchronize()
    assert torch.all(x == 7.0)


# ------------------------------------------------------------------ dge_wp_axis_pairs
@pytest.mark.parametrize("L", [1, 10, 18])
@pytest.mark.parametrize("D", [8, 512])
@pytest.mark.parametrize("n", [1, 3])
def test_wp_axis_pairs(L, D, n):
    """The rows outside [r0, r1) are bit copies of wp; the moved rows are within one ulp of float32(float64(wp) +- float64(h) q): the
    kernel's fma rounds once, the float64 route may round twice."""
    from dge_amd import ops
    wp = R.randn(f"region.wp.{L}.{D}", (L, D), 61)
    q = R.randn(f"region.q.{n}.{D}", (n, D + 3), 62)
    h = float(np.float32(0.3))
    qd = q.cuda()[:, 1:1 + D]          # rows strided
    for r0, r1 in {(0, L), (L // 2, L // 2 + 1), (L // 2, L // 2)}:
        out = ops.wp_axis_pairs(wp.cuda(), qd, r0, r1, h)
        assert ops.last_kernel() == "wp_axis_pairs" and tuple(out.shape) == (2 * n, L, D)
        got = out.cpu().numpy()
        w64, q64 = wp.double().numpy(), q[:, 1:1 + D].double().numpy()
        for j in range(n):
            for half, sign in ((0, 1.0), (1, -1.0)):
                row = got[2 * j + half]
                keep = np.ones(L, dtype=bool)
                keep[r0:r1] = False
                assert np.array_equal(row[keep].view(np.uint32), wp.numpy()[keep].view(np.uint32))
                want = (w64[r0:r1] + sign * h * q64[j]).astype(np.float32)
                ulp = np.spacing(np.abs(want))
                assert np.all(np.abs(row[r0:r1].astype(np.float64) - want.astype(np.float64)) <= ulp)
    from dge_amd._lib import DgeError
    for r0, r1 in ((-1, 1), (0, L + 1), (1, 0)):
        with pytest.raises(DgeError, match="outside"):
            ops.wp_axis_pairs(wp.cuda(), qd, r0, r1, h)


# ------------------------------------------------------------------ dge_matmul_f64acc
@pytest.mark.parametrize("M,N,Kk", [(1, 1, 1), (3, 5, 7), (64, 33, 130), (512, 512, 512)])
@pytest.mark.parametrize("trans_b", [False, True])
def test_matmul_f64acc(M, N, Kk, trans_b):
    """|out - ref| <= 2^-24 |ref| + Kk 2^-53 sum_k |a||b|: the f64 products are exact, the f64 sum carries Kk roundings, and the result
    is rounded once to f32.  Every operand and the result a view with a padded leading dimension; the padding keeps its bits."""
    from dge_amd import ops
    a = R.randn(f"region.mm.a.{M}.{Kk}", (M, Kk + 3), 71)
    b = R.randn(f"region.mm.b.{N}.{Kk}.{trans_b}", (N, Kk + 2) if trans_b else (Kk, N + 2), 72)
    wide = torch.full((M, N + 4), 7.0, device="cuda")
    ad, bd = a.cuda()[:, 2:2 + Kk], (b.cuda()[:, 1:1 + Kk] if trans_b else b.cuda()[:, 1:1 + N])
    out = ops.matmul_f64acc(ad, bd, trans_b=trans_b, out=wide[:, 1:1 + N])
    assert ops.last_kernel() == "matmul_f64acc"
    a64 = a[:, 2:2 + Kk].double().numpy()
    b64 = b[:, 1:1 + Kk].double().numpy().T if trans_b else b[:, 1:1 + N].double().numpy()
    ref = a64 @ b64
    bound = U * np.abs(ref) + Kk * 2.0 ** -53 * (np.abs(a64) @ np.abs(b64))
    got = wide.cpu().numpy()
    err = np.abs(got[:, 1:1 + N].astype(np.float64) - ref)
    assert np.all(err <= bound), float((err / bound).max())
    assert np.all(got[:, :1] == 7.0) and np.all(got[:, 1 + N:] == 7.0)
    assert torch.equal(ops.matmul_f64acc(ad.contiguous(), bd.contiguous(), trans_b=trans_b), out)
    meas(f"region.matmul_f64acc.{M}x{N}x{Kk}.{'t' if trans_b else 'n'}", of_bound=float((err / bound).max()))


def test_matmul_f64acc_refusals():
    from dge_amd import ops
    from dge_amd._lib import DgeError
    a = torch.ones(4, 6, device="cuda")
    for x, y, t in ((a, torch.ones(5, 4, device="cuda"), False), (a, torch.ones(4, 5, device="cuda"), True), (torch.ones(1025, 2, device="cuda"), torch.ones(2, 2, device="cuda"), False),
                    (a.double(), torch.ones(6, 2, device="cuda"), False), (a.cpu(), torch.ones(6, 2), False)):
        with pytest.raises(DgeError):
            ops.matmul_f64acc(x, y, trans_b=t)
