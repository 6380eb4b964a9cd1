"""The Grad-CAM kernels (csrc/gradcam_kernels.hip and relu modes 1 / 2 of maxpool_bwd_kernel in csrc/lpips_kernels.hip), one operation at
a time through the C ABI, against float64 restatements in plain torch / numpy on the same operands (bf16 operands: the bf16-rounded
values), at the shapes the workload runs and the golden run (96 x 96: a 3 x 3 pooled map, a 6 x 6 CAM, C = 64) does not reach.

Bounds.  Selections, copies, arg-max results, minmax and heat are bit-exact.  An f32 sum of n terms gets (n + 1) * 2^-23 * sum |terms|
per output, from the restatement's own terms (+ 2^-8 |ref| for a bf16 output).  A short chain of f32 operations on values in [0, 1]
gets (roundings on the path) * 2^-23, absolute (cam_resize; the mask2cam normalisation carries the magnitudes of its operands, see
_mask2cam_bound).  Where a stage reads an earlier kernel output (cam reads wgt, minmax reads cam, cam_resize reads cam and minmax) the
restatement is fed the kernel's own earlier output.  Every bound prints the measured error beside it (MEAS lines, pytest -rP).

Measured on MI355X, the element closest to its bound over all cases (error of bound; in brackets the largest error of that case):
  adaptive_pool7 8.2e-10 of 7.7e-9 at 5 x 9 (1.2e-7); adaptive_pool7_bwd f32 1.5e-13 of 9.4e-13 at 32 x 32 (1.8e-8), bf16 2.9e-5 of
  3.1e-5 at 7 x 7 (one bf16 rounding of a value just above a power of two); adjoint identity 1.7e-6 of 3.5e-4 at 3 x 3;
  campp_map wgt mode 0 6.0e-9 of 5.9e-7 (1.3e-7), mode 1 6.0e-8 of 2.4e-7 from 1, cam 8.2e-8 of 2.0e-5 (1.5e-7); cam_resize 1.25e-7 of
  1.07e-6 at 8 x 8 -> 256 x 256; mask2cam cam 1.3e-7 of 6.9e-7 at sample 0 of 260 x 256 (bounds 6.8e-7 for sample 0 to 2.2e-6 for
  sample 4); masks at 256 x 224 1.0e-6 of 2e-3.  Everything else is exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gradcam_ref as GR
from tests.conftest import meas
from tests.golden import recipe as R
from tests.test_biggan_kernels_gpu import CDS, U32, _DT, _check, _ep, _windows

pytestmark = pytest.mark.gpu


def _abi():
    from dge_amd import ops
    from dge_amd._lib import DgeError, check, lib
    return ops, lib(), check, DgeError


def _dtc(ops, cd):
    return ops.F32 if cd == "f32" else ops.BF16


def _same_bits(a, b):
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


# ------------------------------------------------------------------ 1. adaptive_pool7 / adaptive_pool7_bwd
_POOL_HW = [(1, 1), (3, 3), (7, 7), (8, 8), (5, 9), (14, 14), (16, 10), (32, 32)]


def _window_sizes(n):
    """sizes of the 7 windows of AdaptiveAvgPool over n: floor(i n / 7) .. ceil((i + 1) n / 7) (for the bounds only)"""
    return torch.tensor([-(-(i + 1) * n // 7) - (i * n) // 7 for i in range(7)], dtype=torch.float64)


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("HW", _POOL_HW)
def test_adaptive_pool7_and_its_adjoint(cd, HW):
    """Forward against F.adaptive_avg_pool2d in float64 (layout c*49 + i*7 + j, f32 output for either input type), adjoint against the
    autograd gradient of the same expression (gy f32, gx in the compute dtype).  1 x 1 and 3 x 3: windows of one pixel (3 x 3: or two),
    49 / 9 of them over every pixel; 7 x 7: the identity; 8 x 8: windows 2 wide that overlap (1 to 4 windows per pixel); 5 x 9, 16 x 10:
    the two axes differ; 14 x 14, 32 x 32: disjoint and overlapping larger windows.  Forward: a sum of n = |window| terms x / n.  Adjoint: m terms gy / n,
    m = the number of windows over the pixel, each behind its own division: (m + 1) * 2^-23 * sum |gy / n|.  f32: <pool(x), gy> =
    <x, pool^T(gy)> on the two kernel outputs, within the sum of the two per-element bounds weighted by the other operand."""
    ops, L, check, _ = _abi()
    Hp, Wp = HW
    for Cc in (8, 40):
        nwin = (_window_sizes(Hp)[:, None] * _window_sizes(Wp)[None, :]).reshape(49).repeat(Cc)      # [C*49]
        for B in (1, 3):
            tags = dict(H=Hp, W=Wp, C=Cc, B=B)
            x = R.randn(f"gk.ap.x.{Hp}.{Wp}.{Cc}.{B}", (B, Hp, Wp, Cc), 81).to(_DT[cd])
            gy = R.randn(f"gk.ap.g.{Hp}.{Wp}.{Cc}.{B}", (B, Cc * 49), 82)
            xa = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
            ref = F.adaptive_avg_pool2d(xa, 7).flatten(1)
            adj = lambda v: torch.autograd.grad(ref, xa, grad_outputs=v.expand_as(ref).contiguous(), retain_graph=True)[0].permute(0, 2, 3, 1)
            gref, gabs, cnt = adj(gy.double()), adj(gy.double().abs()), adj(nwin[None, :])
            assert cnt.min().item() == 1 or min(HW) < 7
            assert cnt.max().item() == {(1, 1): 49, (3, 3): 9, (7, 7): 1, (14, 14): 1, (8, 8): 4}.get(HW, cnt.max().item())
            fbound = (nwin + 1) * U32 * F.adaptive_avg_pool2d(x.double().abs().permute(0, 3, 1, 2), 7).flatten(1)
            gbound = (cnt + 1) * U32 * gabs
            xg, gyg = x.cuda(), gy.cuda()
            y = torch.empty((B, Cc * 49), dtype=torch.float32, device="cuda")
            check(L.dge_adaptive_pool7(ops._p(xg), ops._f32(y), B, Hp, Wp, Cc, _dtc(ops, cd), ops._stream()), "dge_adaptive_pool7")
            gx = torch.empty_like(xg)
            check(L.dge_adaptive_pool7_bwd(ops._f32(gyg), ops._p(gx), B, Hp, Wp, Cc, _dtc(ops, cd), ops._stream()), "dge_adaptive_pool7_bwd")
            y, gx = y.cpu(), gx.cpu()
            _check("adaptive_pool7", y, ref.detach(), fbound, "f32", src=cd, **tags)
            _check("adaptive_pool7_bwd", gx, gref, gbound, cd, **tags)
            if cd == "f32":
                lhs, rhs = (y.double() * gy.double()).sum().item(), (x.double() * gx.double()).sum().item()
                bound = (fbound * gy.double().abs()).sum().item() + (x.double().abs() * gbound).sum().item()
                meas("adaptive_pool7_adjoint_identity", err=abs(lhs - rhs), bound=bound, **tags)
                assert abs(lhs - rhs) <= bound, (tags, lhs, rhs, bound)


# ------------------------------------------------------------------ 2. guided_relu_bwd
# (a, g): a == 0 with g > 0; a > 0 with g == -0.0; a > 0 with g < 0; a == -0.0 with g > 0; a > 0 with g == +0.0; -0.0 in both
_RELU_PLANTS = [(0.0, 1.0), (1.0, -0.0), (1.0, -1.0), (-0.0, 2.0), (1.0, 0.0), (-0.0, -0.0)]


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("chunks", [1, 257, 8192 * 256 + 3])
def test_guided_relu_bwd_is_a_selection(cd, chunks):
    """gpre = (a > 0 and (not guided or g > 0)) ? g : 0, bit for bit (a passed-through -0.0 keeps its sign).  One 16-byte chunk; 257
    chunks (a second, ragged workgroup); 8192 * 256 + 3 chunks: the grid is capped at 8192 workgroups, so the last three chunks are the
    second trip of the grid-stride loop.  The planted pairs sit in the first chunk(s) and, mirrored, in the last ones."""
    ops, L, check, _ = _abi()
    n = chunks * _ep(cd)
    a = torch.relu(R.randn(f"gk.gr.a.{n}", (n,), 83))
    g = R.randn(f"gk.gr.g.{n}", (n,), 84)
    for k, (pa, pg) in enumerate(_RELU_PLANTS):
        if k < n:
            a[k], g[k] = pa, pg
        if n >= 2 * len(_RELU_PLANTS):
            a[n - 1 - k], g[n - 1 - k] = pa, pg
    a, g = a.to(_DT[cd]), g.to(_DT[cd])
    ag, gg = a.cuda(), g.cuda()
    zero = torch.zeros((), dtype=_DT[cd])
    for guided in (0, 1):
        out = torch.empty_like(ag)
        check(L.dge_guided_relu_bwd(ops._p(gg), ops._p(ag), ops._p(out), n, guided, _dtc(ops, cd), ops._stream()), "dge_guided_relu_bwd")
        want = torch.where((a > 0) & ((g > 0) if guided else torch.ones_like(a, dtype=torch.bool)), g, zero)
        assert _same_bits(out.cpu(), want), (cd, chunks, guided)


@pytest.mark.parametrize("cd", CDS)
def test_guided_relu_bwd_refuses_a_partial_chunk(cd):
    ops, L, check, DgeError = _abi()
    ep = _ep(cd)
    t = torch.zeros(2 * ep, dtype=_DT[cd], device="cuda")
    out = torch.empty_like(t)
    with pytest.raises(DgeError, match="guided_relu_bwd"):
        check(L.dge_guided_relu_bwd(ops._p(t), ops._p(t), ops._p(out), ep + 1, 1, _dtc(ops, cd), ops._stream()), "dge_guided_relu_bwd")


# ------------------------------------------------------------------ 3. maxpool2_relu_bwd (relu modes 1 and 2 of maxpool_bwd_kernel)
_TIES_FIRST = [[0.0, 0.0, 0.0, 0.0], [2.0, 2.0, 1.0, 1.0], [1.0, 2.0, 2.0, 0.0], [0.0, 1.0, 2.0, 2.0]]      # window (0,0) of sample 0, channels 0..3
_TIES_LAST = [[2.0, 1.0, 1.0, 2.0], [3.0, 3.0, 3.0, 3.0], [0.0, 2.0, 1.0, 2.0], [1.0, 0.5, 0.5, 1.0]]       # last window of the last sample


def _pool_relu_operands(cd, B, H, W, Cc):
    """x = relu(random) on a grid of halves (exact in bf16, equal maxima inside windows are common) with an all-zero window and positive
    ties at every window position; gy random with a positive value over the zero window and -1, +0.0, -0.0 over three arg-maxima"""
    x = torch.relu(torch.round(2.0 * R.randn(f"gk.mp.x.{B}.{H}.{W}.{Cc}", (B, H, W, Cc), 85, 1.2)) / 2.0)
    gy = R.randn(f"gk.mp.g.{B}.{H}.{W}.{Cc}", (B, H // 2, W // 2, Cc), 86)
    for c, p in enumerate(_TIES_FIRST):
        x[0, 0, 0, c], x[0, 0, 1, c], x[0, 1, 0, c], x[0, 1, 1, c] = p
    gy[0, 0, 0, 0], gy[0, 0, 0, 1], gy[0, 0, 0, 2], gy[0, 0, 0, 3] = 1.5, -1.0, 0.0, -0.0
    if B > 1 or H > 2:
        for c, p in enumerate(_TIES_LAST):
            x[-1, H - 2, W - 2, c], x[-1, H - 2, W - 1, c], x[-1, H - 1, W - 2, c], x[-1, H - 1, W - 1, c] = p
    return x.to(_DT[cd]), gy.to(_DT[cd])


def _pool_relu_restated(gy, x, guided):
    """The first arg-max of every window in the order (0,0), (0,1), (1,0), (1,1), written out (a later element replaces the running
    maximum only when strictly larger); the window's gy goes there when the maximum is > 0 (guided: and gy > 0), +0 everywhere else."""
    B, H, W, Cc = x.shape
    w = _windows(x)                                               # [B,OH,OW,C,4]
    am = torch.zeros(w.shape[:-1], dtype=torch.long)
    mv = w[..., 0].clone()
    for q in (1, 2, 3):
        up = w[..., q] > mv
        am = torch.where(up, torch.full_like(am, q), am)
        mv = torch.where(up, w[..., q], mv)
    zero = torch.zeros((), dtype=x.dtype)
    val = torch.where((mv > 0) & ((gy > 0) if guided else torch.ones_like(mv, dtype=torch.bool)), gy, zero)
    out = torch.where(torch.arange(4) == am[..., None], val[..., None], zero)
    return out.reshape(B, H // 2, W // 2, Cc, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, H, W, Cc).contiguous(), w, am


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("HW", [(2, 2), (4, 4), (6, 10)])
def test_maxpool2_relu_bwd_on_planted_ties(cd, HW):
    """dge_maxpool2_relu_bwd, guided 0 / 1 (relu modes 1 / 2), bit for bit against the restatement above and against the two launches it
    replaces, guided_relu_bwd(maxpool2_bwd(gy, x), x)."""
    ops, L, check, _ = _abi()
    H, W = HW
    ep = _ep(cd)
    for Cc in (ep, 3 * ep):
        for B in (1, 2):
            x, gy = _pool_relu_operands(cd, B, H, W, Cc)
            _, w, am = _pool_relu_restated(gy, x, 0)
            mx = w.amax(dim=-1, keepdim=True)
            tie = ((w == mx) & (mx > 0)).sum(dim=-1) > 1
            assert bool(tie.any()) and bool((w == 0).all(dim=-1).any()) and bool(((gy <= 0) & (mx[..., 0] > 0)).any())
            firsts = set(am[tie].tolist())
            assert firsts >= {0, 1, 2}, firsts                    # (position 3 is never the first of two)
            xg, gyg = x.cuda(), gy.cuda()
            for guided in (0, 1):
                out = torch.empty_like(xg)
                check(L.dge_maxpool2_relu_bwd(ops._p(gyg), ops._p(xg), ops._p(out), B, H, W, Cc, guided, _dtc(ops, cd), ops._stream()),
                      "dge_maxpool2_relu_bwd")
                want = _pool_relu_restated(gy, x, guided)[0]
                assert _same_bits(out.cpu(), want), (cd, HW, Cc, B, guided)
                two, routed = torch.empty_like(xg), ops.maxpool2_bwd(gyg, xg)
                check(L.dge_guided_relu_bwd(ops._p(routed), ops._p(xg), ops._p(two), xg.numel(), guided, _dtc(ops, cd),
                                            ops._stream()), "dge_guided_relu_bwd")
                assert _same_bits(out.cpu(), two.cpu()), (cd, HW, Cc, B, guided)


@pytest.mark.parametrize("cd", CDS)
def test_maxpool2_relu_bwd_refuses_odd_sizes(cd):
    ops, L, check, DgeError = _abi()
    ep = _ep(cd)
    for H, W in ((3, 2), (2, 3)):
        x = torch.zeros((1, H, W, ep), dtype=_DT[cd], device="cuda")
        gy = torch.zeros((1, 1, 1, ep), dtype=_DT[cd], device="cuda")
        out = torch.empty_like(x)
        with pytest.raises(DgeError, match="even"):
            check(L.dge_maxpool2_relu_bwd(ops._p(gy), ops._p(x), ops._p(out), 1, H, W, ep, 1, _dtc(ops, cd), ops._stream()),
                  "dge_maxpool2_relu_bwd")


# ------------------------------------------------------------------ 4. class_target (coupled form) / class_target_rows
def _vote_logits(B, K):
    """Values on a grid of halves.  K >= 10: row 0 holds its maximum twice (columns 1 and K - 1: the first one wins); B >= 4: rows
    1 .. 2m (m = (B - 2) // 2) vote for class 7 and class 3 in turn, m votes each - the smaller index wins the vote -, a left-over row
    votes for 9; the last row of B >= 2 is constant (its arg-max is 0)."""
    lg = torch.round(2.0 * R.randn(f"gk.ct.{B}.{K}", (B, K), 87)) / 2.0
    if K >= 10:
        lg[0, 1] = lg[0, K - 1] = 10.0
        if B >= 4:
            m = (B - 2) // 2
            rows = torch.arange(1, 1 + 2 * m)
            lg[rows[rows % 2 == 1], 7] = 20.0
            lg[rows[rows % 2 == 0], 3] = 20.0
            lg[1 + 2 * m:B - 1, 9] = 20.0
    if B >= 2:
        lg[B - 1] = 0.5
    return lg


def _vote_index(B, K):
    """Given class ids: B >= 4 and K >= 10: m votes each for 7 and 3 (7 first), the rest for 9 and 0; else seeded random ids."""
    if B >= 4 and K >= 10:
        m = (B - 2) // 2
        idx = np.full(B, 9, dtype=np.int32)
        idx[0:2 * m:2], idx[1:2 * m:2], idx[B - 1] = 7, 3, 0
        return idx
    return np.random.RandomState(1000 * B + K).randint(0, K, size=B).astype(np.int32)


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("B,K", [(1, 1), (1, 40), (1, 1000), (3, 1), (3, 40), (3, 1000), (257, 1), (257, 40), (257, 1000), (1024, 1), (1024, 40)])
def test_class_target_vote_against_numpy(B, K, given):
    """index_out = [np.argmax(np.bincount(rows)), rows...] with rows = np.argmax(logits, axis=1) or the given ids; glogits is exactly
    float32(1) / float32(B) in column index_max and 0 elsewhere.  B = 257 and 1024: the row loop of the 256 threads takes more trips."""
    ops, L, check, _ = _abi()
    lg = _vote_logits(B, K)
    rows = _vote_index(B, K) if given else np.argmax(lg.numpy(), axis=1).astype(np.int32)
    votes = np.bincount(rows)
    imax = int(np.argmax(votes))
    if K >= 10:
        assert given or rows[0] == 1
        if B >= 4:
            assert imax == 3 and votes[3] == votes[7] and (votes[[k for k in range(len(votes)) if k not in (3, 7)]] < votes[3]).all()
    if B >= 2 and not given:
        assert rows[B - 1] == 0
    out = torch.empty(1 + B, dtype=torch.int32, device="cuda")
    g = torch.empty((B, K), dtype=torch.float32, device="cuda")
    idx_in = torch.from_numpy(rows).cuda() if given else None
    lgg = lg.cuda()                     # (every device operand is held by a name until the results are back)
    check(L.dge_class_target(ops._f32(lgg), ops._p(idx_in), ops._p(out), ops._f32(g), B, K, ops._stream()), "dge_class_target")
    assert out.cpu().tolist() == [imax] + rows.tolist()
    want = np.zeros((B, K), dtype=np.float32)
    want[:, imax] = np.float32(1) / np.float32(B)
    assert np.array_equal(g.cpu().numpy(), want)


def test_class_target_refuses_more_rows_than_its_workgroup_holds():
    ops, L, check, DgeError = _abi()
    lg = torch.zeros((1025, 1), dtype=torch.float32, device="cuda")
    out = torch.empty(1026, dtype=torch.int32, device="cuda")
    g = torch.empty_like(lg)
    with pytest.raises(DgeError, match="class_target"):
        check(L.dge_class_target(ops._f32(lg), None, ops._p(out), ops._f32(g), 1025, 1, ops._stream()), "dge_class_target")


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 1000])
def test_class_target_rows_against_numpy(K, B, given):
    """One wave per row: K < 64 leaves idle lanes, K = 65 gives lane 0 a second trip, B = 5 a ragged second workgroup.  Equal maxima in
    two lanes with the smaller index in the HIGHER lane (columns 64 and 1: lanes 0 and 1), and on a grid of halves further equal maxima
    wherever the seed puts them; the last row of B = 5 is constant.  glogits is exactly one-hot."""
    ops, L, check, _ = _abi()
    lg = torch.round(2.0 * R.randn(f"gk.cr.{B}.{K}", (B, K), 88)) / 2.0
    if K >= 65:
        lg[0, 64] = lg[0, 1] = 9.0
    elif K >= 3:
        lg[0, K - 1] = lg[0, 2] = 9.0
    if B > 1:
        if K == 1000:
            lg[1, 700] = lg[1, 130] = 9.0
        lg[B - 1] = -1.5
    rows = (np.random.RandomState(77 * B + K).randint(0, K, size=B) if given else np.argmax(lg.numpy(), axis=1)).astype(np.int32)
    if not given and K >= 3:
        assert rows[0] == (1 if K >= 65 else 2) and (B == 1 or rows[B - 1] == 0)
    out = torch.empty(B, dtype=torch.int32, device="cuda")
    g = torch.empty((B, K), dtype=torch.float32, device="cuda")
    idx_in = torch.from_numpy(rows).cuda() if given else None
    lgg = lg.cuda()
    check(L.dge_class_target_rows(ops._f32(lgg), ops._p(idx_in), ops._p(out), ops._f32(g), B, K, ops._stream()), "dge_class_target_rows")
    assert out.cpu().tolist() == rows.tolist()
    want = np.zeros((B, K), dtype=np.float32)
    want[np.arange(B), rows] = 1.0
    assert np.array_equal(g.cpu().numpy(), want)


def test_select_target_refuses_an_out_of_range_host_index(monkeypatch):
    """The winning class id addresses a row of the classifier weight (gather_row_kernel): a host-side id outside [0, K) is a ValueError
    before anything is launched (no kernel ever sees it here); the edges 0 and K - 1 pass."""
    from dge_amd import grad_cam as G
    cfg = R.GRADCAM_CFG
    K = cfg["classes"]
    net = G.VGG16(cfg["widths"], cfg["fc"], K, compute_dtype="f32")
    logits = torch.zeros((1, K), dtype=torch.float32, device="cuda")
    for good in (0, K - 1):
        idx, _ = net.select_target(logits, [good])
        assert idx.cpu().tolist() == [good, good]
    monkeypatch.setattr(G, "lib", lambda: pytest.fail("select_target reached the library with an out-of-range index"))
    for bad in ([K], [-1], np.array([K]), torch.tensor([-1])):
        with pytest.raises(ValueError, match="index must lie in"):
            net.select_target(logits, bad)
    two = torch.zeros((2, K), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="index must lie in"):
        net.select_target(two, [0, K], groups=2)


# ------------------------------------------------------------------ 5. gather_row / gather_rows
@pytest.mark.parametrize("B", [1, 3, 300])
def test_gather_row_and_gather_rows_are_copies(B):
    """y[b] = float32(scale) * w[index[0]] (one f32 product) and y[b] = w[index[b]], the ids read from a device tensor.  B * I = 300 *
    4096 is more than the 1024 workgroups of the launch cover at once: the stride loop takes further trips."""
    ops, L, check, _ = _abi()
    O = 7
    for I in (1, 37, 4096):
        w = R.randn(f"gk.ga.{I}", (O, I), 89)
        wg = w.cuda()
        scale = 1.0 / B
        first = torch.tensor([5] + [2] * B, dtype=torch.int32).cuda()       # [index_max, per-row ids]: element 0 alone is read
        y = torch.empty((B, I), dtype=torch.float32, device="cuda")
        check(L.dge_gather_row(ops._f32(wg), ops._p(first), ops._f32(y), B, I, scale, ops._stream()), "dge_gather_row")
        want = np.broadcast_to(np.float32(scale) * w.numpy()[5], (B, I))
        assert want.dtype == np.float32 and np.array_equal(y.cpu().numpy(), want), (B, I)
        ids = np.random.RandomState(31 * B + I).randint(0, O, size=B).astype(np.int32)
        idg = torch.from_numpy(ids).cuda()
        y = torch.empty((B, I), dtype=torch.float32, device="cuda")
        check(L.dge_gather_rows(ops._f32(wg), ops._p(idg), ops._f32(y), B, I, ops._stream()), "dge_gather_rows")
        assert np.array_equal(y.cpu().numpy(), w.numpy()[ids]), (B, I)


# ------------------------------------------------------------------ 6. campp_map
def _campp_run(cd, mode, g, f):
    ops, L, check, _ = _abi()
    B, HW, Cc = g.shape
    gg, fg = g.cuda(), f.cuda()
    wgt = torch.empty((B, Cc), dtype=torch.float32, device="cuda")
    cam = torch.empty((B, HW), dtype=torch.float32, device="cuda")
    mm = torch.empty((B, 2), dtype=torch.float32, device="cuda")
    check(L.dge_campp_map(ops._p(gg), ops._p(fg), ops._f32(wgt), ops._f32(cam), ops._f32(mm), B, HW, Cc, mode, _dtc(ops, cd),
                          ops._stream()), "dge_campp_map")
    return wgt.cpu(), cam.cpu(), mm.cpu()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cd", CDS)
def test_campp_map_weights_sum_and_extrema(cd, mode):
    """(C, HW, B): one chunk of channels and one pixel; C = 64 with HW = 15 (one of the 16 pixel waves idle); C = 72 (a tail channel
    block of 8 lanes) with HW = 36 and 256; C = 512 (8 channel blocks) with HW = 64 and 15.  Channel 1 has no positive gradient (one
    of them exactly 0).  wgt: mode 1 exactly 0 where no gradient is positive, else s * (1 / s): two roundings around 1; mode 0 the mean,
    HW terms.  cam from the kernel's own wgt (C terms; mode 0 clamps at 0, which does not widen an error).  minmax: the extrema of the
    kernel's own cam, exact."""
    ep = _ep(cd)
    for Cc, HW, B in [(ep, 1, 1), (64, 15, 3), (72, 36, 1), (512, 64, 3), (72, 256, 3), (512, 15, 1)]:
        tags = dict(C=Cc, HW=HW, B=B, mode=mode)
        g = R.randn(f"gk.cm.g.{Cc}.{HW}.{B}", (B, HW, Cc), 90)
        g[:, :, 1] = -g[:, :, 1].abs()
        g[0, 0, 1] = 0.0
        g = g.to(_DT[cd])
        f = torch.relu(R.randn(f"gk.cm.f.{Cc}.{HW}.{B}", (B, HW, Cc), 91)).to(_DT[cd])
        wgt, cam, mm = _campp_run(cd, mode, g, f)
        g64, f64 = g.double(), f.double()
        if mode == 1:
            pos = (g64 > 0).any(dim=1)
            assert not bool(pos[:, 1].any()) and (bool(pos.any()) or Cc * HW * B < 64)
            assert bool((wgt[~pos] == 0).all()), tags
            err = (wgt[pos].double() - 1.0).abs().max().item() if bool(pos.any()) else 0.0
            meas("campp_weight_pp", cd=cd, err=err, bound=2 * U32, **tags)                # 1 / s and s * (1 / s): two roundings
            assert err <= 2 * U32, (tags, err)
        else:
            _check("campp_weight_mean", wgt, g64.mean(dim=1), (HW + 1) * U32 * g64.abs().sum(dim=1) / HW, "f32", src=cd, **tags)
        prod = f64 * wgt.double()[:, None, :]
        ref = prod.sum(dim=-1)
        _check("campp_sum", cam, ref.clamp(min=0) if mode == 0 else ref, (Cc + 1) * U32 * prod.abs().sum(dim=-1), "f32", src=cd, **tags)
        assert torch.equal(mm[:, 0], cam.min(dim=1).values) and torch.equal(mm[:, 1], cam.max(dim=1).values), tags


@pytest.mark.parametrize("cd", CDS)
def test_campp_map_refuses_a_partial_channel_chunk(cd):
    _, _, _, DgeError = _abi()
    t = torch.zeros((1, 2, 2 * _ep(cd)), dtype=_DT[cd])
    with pytest.raises(DgeError, match="campp_map"):
        _campp_run(cd, 1, t[:, :, :_ep(cd) + 2].contiguous(), t[:, :, :_ep(cd) + 2].contiguous())


# ------------------------------------------------------------------ 7. cam_resize
_RESIZE = [((6, 6), (96, 96)), ((7, 7), (224, 224)), ((8, 8), (256, 256)), ((1, 1), (32, 32)), ((3, 5), (32, 64)), ((9, 7), (5, 4))]


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shape", _RESIZE)
def test_cam_resize_against_the_cv2_restatement(shape, B):
    """(cam - lo) / (hi - lo) and OpenCV's INTER_LINEAR taps: ratios 16 (the golden run's), 32, 32 again from 8 x 8, a 1 x 1 source,
    two ratios at once (32 / 3 and 64 / 5) and a down-scale; cam, lo and hi are campp_map's own outputs.  A row with hi == lo (the second
    row of the 3 x 5 case, whose features are zero, and every row of a 1 x 1 source) is 0 / 0 on both sides: all NaN, nothing else asked.
    Roundings on the longest path, values in [0, 1]: c - lo, hi - lo, the division (3); 1 - ax, v * (1 - ax), top's addition (3);
    1 - ay, top * (1 - ay), the last addition (3): 9 * 2^-23, absolute."""
    ops, L, check, _ = _abi()
    (h, w), (H, W) = shape
    g = R.randn(f"gk.rs.g.{h}.{w}.{B}", (B, h * w, 64), 92)
    f = torch.relu(R.randn(f"gk.rs.f.{h}.{w}.{B}", (B, h * w, 64), 93))
    if B == 2 and (h, w) == (3, 5):
        f[1] = 0.0
    _, cam, mm = _campp_run("f32", 1, g, f)
    mask = torch.empty((B, 1, H, W), dtype=torch.float32, device="cuda")
    camg, mmg = cam.cuda(), mm.cuda()
    check(L.dge_cam_resize(ops._f32(camg), ops._f32(mmg), ops._f32(mask), B, h, w, H, W, ops._stream()), "dge_cam_resize")
    mask = mask.cpu().numpy()
    judged = 0
    for b in range(B):
        lo, hi = float(mm[b, 0]), float(mm[b, 1])
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = GR.cv2_resize_linear((cam[b].double().numpy().reshape(h, w) - lo) / (hi - lo), (W, H))
        if hi == lo:
            assert np.isnan(ref).all() and np.isnan(mask[b, 0]).all(), (shape, b)
            continue
        judged += 1
        assert ref.min() >= 0.0 and ref.max() <= 1.0 + 1e-12
        err = float(np.abs(mask[b, 0].astype(np.float64) - ref).max())
        meas("cam_resize", err=err, bound=9 * U32, h=h, w=w, H=H, W=W, B=B, b=b)
        assert err <= 9 * U32, (shape, b, err)
    assert judged == (0 if h * w == 1 else (1 if (B == 2 and (h, w) == (3, 5)) else B))


# ------------------------------------------------------------------ 8. mask2cam (coupled form)
def _mask2cam_restated(heat, img):
    """grad_cam.py:241-250 in float64: sample i becomes heat + img, is shifted by the minimum of the WHOLE array as it stands (samples
    < i normalised, samples > i the raw images) and divided by its own maximum.  Also, per sample, the three candidates of that
    minimum (its own, the normalised earlier samples', the raw later images'), the span and the largest magnitude that entered."""
    B = img.shape[0]
    cam = img.clone()
    info = []
    for i in range(B):
        cam[i] = heat[i] + img[i]
        own = cam[i].min().item()
        done = cam[:i].min().item() if i else float("inf")
        raw = cam[i + 1:].min().item() if i + 1 < B else float("inf")
        m = cam.min().item()
        assert m == min(own, done, raw)
        span = cam[i].max().item() - m
        info.append(dict(own=own, done=done, raw=raw, span=span, mag=max(cam[i].abs().max().item(), abs(m))))
        cam[i] = (cam[i] - m) / span
    return cam, info


def _mask2cam_bound(info):
    """E_i, absolute, for the normalised sample i = (cv - m) / (xc - m) in [0, 1], u = 2^-23 per rounding, A = the largest magnitude:
    cv = heat + img is one rounding (u A); m is a minimum (1-Lipschitz) over such values, raw image values (exact) and the normalised
    earlier samples: e_m = max(u A, E_j, j < i); numerator and span each carry u A + e_m and their own rounding (u * span at most); the
    quotient q <= 1 adds one more: E_i = (2 (u A + e_m) + 2 u span) / span + u = 2 (u A + e_m) / span + 3 u.  It grows with i."""
    E = []
    for d in info:
        e_m = max([U32 * d["mag"]] + E)
        E.append(2.0 * (U32 * d["mag"] + e_m) / d["span"] + 3.0 * U32)
    return E


@pytest.mark.parametrize("imgs", ["pm1", "shifted"])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("HW", [(16, 16), (20, 13), (260, 256)])
def test_mask2cam_heat_exact_and_sequential_normalisation(HW, B, imgs):
    """mask = (k + 0.5) / 255 for random k in 0 .. 254, with 0.0 and 1.0 planted: uint8(255 * mask) is k with a margin of a half (checked
    below in f32 for the values used), so heat = float32(lut[k]) / float32(255) for EVERY pixel, bit for bit.  16 x 16: one workgroup
    per sample; 20 x 13: a second one with 4 pixels; 260 x 256: more pixels than the 256 workgroups cover at once.  Images in [-1, 1]
    with -1 in samples >= 1 and nothing below -0.9 in sample 0: the raw minimum of a later sample decides sample 0's shift; images in
    [0.5, 1.5]: the normalised minimum of sample 0 decides sample 1's."""
    from dge_amd import grad_cam as G
    ops, L, check, _ = _abi()
    H, W = HW
    n = H * W
    k = np.random.RandomState(n + B).randint(0, 255, size=(B, n))
    mask = ((k + 0.5) / 255.0).astype(np.float32)
    mask[0, 0], k[0, 0] = 0.0, 0
    mask[0, 1], k[0, 1] = 1.0, 255
    assert np.array_equal((np.float32(255) * mask).astype(np.int64), k)
    z = R.randn(f"gk.mc.{imgs}.{B}.{n}", (B, 3, n), 94)
    if imgs == "pm1":
        img = (0.5 * z).clamp(-0.9, 1.0)
        img[1:, 2, n - 1] = -1.0
    else:
        img = 0.5 + (0.5 + 0.25 * z).clamp(0.0, 1.0)
    lut = torch.from_numpy(G._jet_table()).cuda().contiguous()
    maskg, imgg = torch.from_numpy(mask).cuda(), img.cuda()
    heat, cam = torch.empty((B, 3, n), dtype=torch.float32, device="cuda"), torch.empty((B, 3, n), dtype=torch.float32, device="cuda")
    part = torch.empty((B, L.dge_mask2cam_blocks(n), 3), dtype=torch.float32, device="cuda")
    coef = torch.empty((B, 2), dtype=torch.float32, device="cuda")
    check(L.dge_mask2cam(ops._f32(maskg), ops._f32(imgg), ops._p(lut), ops._f32(heat), ops._f32(cam),
                         ops._f32(part), ops._f32(coef), B, n, ops._stream()), "dge_mask2cam")
    heat, cam = heat.cpu(), cam.cpu()
    lutf = GR.jet_lut()[:, ::-1].astype(np.float32) / np.float32(255)              # the oracle's table is B,G,R
    want = np.transpose(lutf[k], (0, 2, 1))                                          # [B,n,3] -> [B,3,n]
    assert np.array_equal(heat.numpy(), want), (HW, B)
    ref, info = _mask2cam_restated(heat.double(), img.double())
    if B > 1:
        d = info[0] if imgs == "pm1" else info[1]
        assert (d["raw"] < min(d["own"], d["done"])) if imgs == "pm1" else (d["done"] < min(d["own"], d["raw"])), d
    E = _mask2cam_bound(info)
    assert E[-1] < 1e-4 and (B == 1 or max(E[1:]) > E[0])           # still far below what a wrong shift moves (0.01 and more)
    bound = torch.tensor(E, dtype=torch.float64)[:, None, None].expand_as(ref)
    _check("mask2cam_cam", cam, ref, bound, "f32", H=H, W=W, B=B, imgs=imgs, bound_first=E[0], bound_last=E[-1])


# ------------------------------------------------------------------ 9. one integration case off the square
def test_masks_at_256x224_against_the_cpu_restatement():
    """The narrow VGG16 of the golden run on two 256 x 224 images, f32, guided: an 8 x 7 pooled map (overlapping windows along one axis,
    the identity along the other) and a 16 x 14 CAM resized by 16 to 256 x 224.  The class is passed explicitly (the restatement's own
    vote) so that near-tied logits cannot reorder; tolerance as in test_gradcam.py: 2e-3 on masks in [0, 1] (f32 accumulation order of
    the 13 convs)."""
    from dge_amd import grad_cam as G
    cfg = R.GRADCAM_CFG
    ref_net = GR.VGG16Ref(cfg["widths"], cfg["fc"], cfg["classes"])
    sd = GR.seeded_state({k: list(v.shape) for k, v in ref_net.state_dict().items()}, cfg["seed"])
    imgs = R.gradcam_images("a", 2, 256, 224)
    ref_pp, index_max = GR.grad_cam_pp(sd, imgs, None, guided=True, plain=False)[:2]
    index = [index_max] * 2
    ref_plain = GR.grad_cam_pp(sd, imgs, index, guided=True, plain=True)[0]
    net = G.VGG16(cfg["widths"], cfg["fc"], cfg["classes"], compute_dtype="f32")
    net.load_state_dict(sd)
    net = net.cuda()
    gcpp = G.GradCamPlusPlus(net, net.final_layer)
    G.GuidedBackPropagation(net)
    plain = G.GradCAM(net, net.final_layer)
    mask = gcpp(imgs.cuda(), index)
    assert tuple(gcpp.feature.shape) == (2, 16, 14, 64) and tuple(mask.shape) == (2, 1, 256, 224)
    assert gcpp.index.cpu().tolist() == [index_max] * 3
    for name, got, ref in (("gradcampp", mask, ref_pp), ("gradcam", plain(imgs.cuda(), index), ref_plain)):
        err = float(np.abs(got.cpu().numpy() - ref.numpy()).max())
        meas("mask_256x224_" + name, err=err, bound=2e-3)
        assert err < 2e-3, (name, err)
