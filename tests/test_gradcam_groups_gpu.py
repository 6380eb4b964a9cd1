"""Group forms of the attention pass (csrc/gradcam_kernels.hip: dge_class_target_groups, dge_gather_row_groups, dge_mask2cam_groups),
the whole-array min-max normalisation (csrc/metrics_kernels.hip: dge_minmax_unit) and GradCAM.with_input_gradient_pair, which puts
the two image batches of a mis-align iteration through VGG16 once.

The three group kernels are judged to the bit against the batch forms they generalise (dge_class_target, dge_gather_row,
dge_mask2cam) on every group's slice.  The pair pass is judged against two with_input_gradient calls with the bounds
tests/test_gradcam.py uses against the reference for the same quantities (masks 2e-3 absolute, gradients 3e-3 of the maximum): its
conv launches see twice the rows and may tile differently, so bit equality is not asked of it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.golden import recipe as R
from oracle import gradcam_ref as GR

pytestmark = pytest.mark.gpu
CFG = R.GRADCAM_CFG


def _call(name, *args):
    from dge_amd._lib import lib, check
    check(getattr(lib(), name)(*args), name)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    from dge_amd.ops import _stream
    return _stream()


# ------------------------------------------------------------------------------------------------ dge_class_target_groups
def _class_target(logits, index_in):
    N, K = logits.shape
    out = torch.full((1 + N,), -7, dtype=torch.int32, device="cuda")
    g = torch.full_like(logits, float("nan"))
    _call("dge_class_target", _ptr(logits), _ptr(index_in), _ptr(out), _ptr(g), N, K, _stream())
    return out, g


def _class_target_groups(logits, index_in, G):
    B, K = logits.shape
    N = B // G
    out = torch.full((G, 1 + N), -7, dtype=torch.int32, device="cuda")      # not pre-zeroed: every element must be written
    g = torch.full_like(logits, float("nan"))
    _call("dge_class_target_groups", _ptr(logits), _ptr(index_in), _ptr(out), _ptr(g), G, N, K, _stream())
    return out, g


def _assert_groups_equal_slices(logits, index_in, G):
    B = logits.shape[0]
    N = B // G
    out, g = _class_target_groups(logits, index_in, G)
    for k in range(G):
        sl = slice(k * N, (k + 1) * N)
        o1, g1 = _class_target(logits[sl].contiguous(), None if index_in is None else index_in[sl].contiguous())
        assert torch.equal(out[k], o1), (k, out[k].tolist(), o1.tolist())
        assert torch.equal(g[sl].view(torch.int32), g1.view(torch.int32)), k
    return out.cpu().tolist(), g.cpu().numpy()


def _crafted(G, N):
    """K = 5 logits with the cases that can go wrong: a row with two equal maxima (first wins), a two-way tie of the vote inside a
    group (smaller class id wins) and, with N = 3, a plain majority in the other group."""
    K = 5
    rows = {
        "c4": [0.1, 0.0, -1.0, 0.3, 2.0],          # class 4
        "c1": [0.0, 1.5, -0.5, 1.0, 0.2],          # class 1
        "c1c3": [0.2, 0.9, 0.1, 0.9, -3.0],        # maxima at 1 and 3: the first, 1
        "c2": [-1.0, -2.0, -0.5, -0.7, -0.9],      # class 2, all negative
        "c0c4": [7.0, 1.0, 2.0, 3.0, 7.0],         # maxima at 0 and 4: 0
    }
    if (G, N) == (2, 3):
        names = ["c4", "c1", "c2",                 # votes 4, 1, 2: a three-way tie, smallest id 1
                 "c4", "c1c3", "c1"]               # votes 4, 1, 1: majority 1
        want = [[1, 4, 1, 2], [1, 4, 1, 1]]
    else:
        names = ["c4", "c1",                       # tie 4 / 1 -> 1
                 "c2", "c0c4",                     # tie 2 / 0 -> 0
                 "c1c3", "c1"]                     # 1, 1 -> 1
        want = [[1, 4, 1], [0, 2, 0], [1, 1, 1]]
    return torch.tensor([rows[n] for n in names], dtype=torch.float32, device="cuda"), want, K


@pytest.mark.parametrize("G,N", [(2, 3), (3, 2)])
def test_class_target_groups_crafted_ties_equal_the_batch_form_on_every_slice(G, N):
    logits, want, K = _crafted(G, N)
    got, g = _assert_groups_equal_slices(logits, None, G)
    assert got == want
    for k in range(G):
        ref = np.zeros((N, K), np.float32)
        ref[:, want[k][0]] = np.float32(1.0) / np.float32(N)
        assert np.array_equal(g[k * N:(k + 1) * N], ref)
    # explicit class ids: the vote runs on them, the logits are not looked at
    idx = torch.tensor(([3, 0, 3, 2, 2, 4] if N == 3 else [3, 0, 2, 2, 4, 1]), dtype=torch.int32, device="cuda")
    got, _ = _assert_groups_equal_slices(logits, idx, G)
    assert got == ([[3, 3, 0, 3], [2, 2, 2, 4]] if N == 3 else [[0, 3, 0], [2, 2, 2], [1, 4, 1]])


@pytest.mark.parametrize("mode", ["default", "deterministic"])
def test_class_target_groups_k1000_same_bits_in_both_reduction_modes(mode):
    from dge_amd import ops
    logits = R.randn("groups.logits", (16, 1000), 0).cuda()
    logits[3, 17] = logits[3].max() + 1.0
    logits[5, 17] = logits[5].max() + 1.0            # group 0 (rows 0..7) gets a majority; group 1's vote is whatever bincount says
    was = ops.is_deterministic()
    ops.set_deterministic(mode == "deterministic")
    try:
        got, g = _assert_groups_equal_slices(logits, None, 2)
    finally:
        ops.set_deterministic(was)
    lg = logits.cpu().numpy()
    for k in range(2):
        rows = lg[k * 8:(k + 1) * 8].argmax(1)
        assert got[k][1:] == rows.tolist()
        assert got[k][0] == int(np.argmax(np.bincount(rows)))           # grad_cam.py:166-170
    assert got[0][0] == 17
    ref = (np.arange(1000)[None, :] == np.repeat([got[0][0], got[1][0]], 8)[:, None]).astype(np.float32) * np.float32(0.125)
    assert np.array_equal(g, ref)


# ------------------------------------------------------------------------------------------------ dge_gather_row_groups
@pytest.mark.parametrize("G,N,I", [(2, 3, 128), (3, 2, 37), (2, 8, 4096)])
def test_gather_row_groups_equals_gather_row_on_every_slice(G, N, I):
    O = 11
    w = R.randn("groups.w6", (O, I), 0).cuda()
    index = torch.full((G, 1 + N), 5, dtype=torch.int32, device="cuda")
    index[:, 0] = torch.tensor([9, 2, 10][:G], dtype=torch.int32)         # only the group's index_max is read
    scale = 1.0 / N
    y = torch.full((G * N, I), float("nan"), device="cuda")
    _call("dge_gather_row_groups", _ptr(w), _ptr(index), _ptr(y), G, N, I, C.c_float(scale), _stream())
    for k in range(G):
        y1 = torch.full((N, I), float("nan"), device="cuda")
        _call("dge_gather_row", _ptr(w), _ptr(index[k].contiguous()), _ptr(y1), N, I, C.c_float(scale), _stream())
        assert torch.equal(y[k * N:(k + 1) * N].view(torch.int32), y1.view(torch.int32)), k
        assert torch.equal(y1[0], (w[int(index[k, 0])] * np.float32(scale)))


# ------------------------------------------------------------------------------------------------ dge_mask2cam_groups
@pytest.mark.parametrize("H", [32, 64])          # 4 and 16 partial blocks per row
def test_mask2cam_groups_restarts_the_recurrence_at_the_group_seam(H):
    from dge_amd import grad_cam as G
    N, groups = 3, 2
    # clearly different ranges, the narrow one first: run across the seam, the recurrence takes group 0's minimum from group 1's
    # raw images (about -1 instead of about -0.4)
    imgs = torch.cat((0.4 * R.gradcam_images("a", N, H, H), R.gradcam_images("b", N, H, H))).cuda()
    mask = torch.rand((groups * N, 1, H, H), generator=torch.Generator().manual_seed(5)).cuda()
    assert G.lib().dge_mask2cam_blocks(H * H) == H * H // 256
    heat, cam = G.mask2cam(mask, imgs, groups=groups)
    for k in range(groups):
        sl = slice(k * N, (k + 1) * N)
        h1, c1 = G.mask2cam(mask[sl], imgs[sl])
        assert torch.equal(heat[sl].view(torch.int32), h1.view(torch.int32)), k
        assert torch.equal(cam[sl].view(torch.int32), c1.view(torch.int32)), k
    hb, cb = G.mask2cam(mask, imgs)                    # one batch of six: the recurrence runs on across the seam
    assert torch.equal(hb, heat)                       # (the heat map is per pixel)
    assert not torch.equal(cb, cam)
    assert float((cb[:N] - cam[:N]).abs().max()) > 1e-3          # the first group's minimum reaches into the second group's images
    with pytest.raises(ValueError):
        G.mask2cam(mask, imgs, groups=4)
    with pytest.raises(ValueError):
        G.mask2cam(mask, imgs, rows=True, groups=2)


# ------------------------------------------------------------------------------------------------ dge_minmax_unit
def _ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib).max()


@pytest.mark.parametrize("shape", [(4, 3, 32, 32), (1000 * 256 + 77,), (5,)])
def test_minmax_unit_matches_numpy_and_hits_zero_and_one_exactly(shape):
    from dge_amd import infer, ops
    x = R.randn("groups.minmax", shape, 0, 3.0)
    ref = x.numpy().copy()
    ref -= np.max(np.min(ref), 0)                      # the scripts' lines, on float32 as there
    ref /= np.max(ref)
    ops.KERNEL_LOG = log = []
    try:
        y = infer.minmax_unit(x.cuda())
    finally:
        ops.KERNEL_LOG = None
    assert [n for n, _ in log] == ["minmax_unit"]
    got = y.cpu().numpy()
    assert got.shape == ref.shape and _ulps(got, ref) <= 1
    assert got.min() == 0.0 and got.max() == 1.0
    was = ops.is_deterministic()
    ops.set_deterministic(not was)
    try:
        assert torch.equal(infer.minmax_unit(x.cuda()), y)
    finally:
        ops.set_deterministic(was)


# ------------------------------------------------------------------------------------------------ the pair pass
def _net(cd="f32"):
    from dge_amd import grad_cam as G
    net = GR.VGG16Ref(CFG["widths"], CFG["fc"], CFG["classes"])
    shapes = {k: list(v.shape) for k, v in net.state_dict().items()}
    m = G.VGG16(CFG["widths"], CFG["fc"], CFG["classes"], compute_dtype=cd)
    m.load_state_dict(GR.seeded_state(shapes, CFG["seed"]))
    return G, m.cuda()


def _logged(fn, monkeypatch=None):
    """-> (result, KERNEL_LOG names, calls of the conv-family ops as (op, input shape)).  ops.conv2d does not write to KERNEL_LOG
    (only the entry points that select among kernel instantiations do), so the conv sequence is traced at the ops layer."""
    from dge_amd import ops
    calls = []
    if monkeypatch is not None:
        for name in ("conv2d", "maxpool2", "linear", "linear_t"):
            def f(*a, _orig=getattr(ops, name), _name=name, **kw):
                calls.append((_name, tuple(a[0].shape)))
                return _orig(*a, **kw)
            monkeypatch.setattr(ops, name, f)
    ops.KERNEL_LOG = log = []
    try:
        out = fn()
    finally:
        ops.KERNEL_LOG = None
        if monkeypatch is not None:
            monkeypatch.undo()
    return out, [n for n, _ in log], calls


# seeds checked on the CPU with oracle/gradcam_ref.py (GR.grad_cam_pp's logits): every row's top-two margin is >= 0.1 of the largest
# |logit| at both shapes, a hundred times the precondition asserted below
@pytest.mark.parametrize("N,H,W", [(2, 32, 32), (3, 64, 32)])
def test_pair_pass_matches_two_separate_passes(N, H, W, monkeypatch):
    G, net = _net()
    gcpp = G.GradCamPlusPlus(net, net.final_layer)
    with pytest.raises(G.DgeError):
        gcpp.with_input_gradient_pair(torch.zeros(1, 3, 32, 32).cuda(), torch.zeros(1, 3, 32, 32).cuda())    # not guided yet
    G.GuidedBackPropagation(net)
    imgs1, imgs2 = R.gradcam_images("a", N, H, W).cuda(), R.gradcam_images("b", N, H, W).cuda()
    sep, idx, logs = [], [], []
    for imgs in (imgs1, imgs2):
        lg = net(imgs).cpu().numpy()
        srt = np.sort(lg, axis=1)
        assert ((srt[:, -1] - srt[:, -2]) >= 1e-3 * np.abs(lg).max()).all(), "precondition: near-tied logits, choose other seeds"
        out, names, calls = _logged(lambda: gcpp.with_input_gradient(imgs), monkeypatch)
        sep.append(out)
        idx.append(gcpp.index.cpu().tolist())
        logs.append((names, calls))
    (m1, g1, m2, g2), names, calls = _logged(lambda: gcpp.with_input_gradient_pair(imgs1, imgs2), monkeypatch)
    assert gcpp.index.cpu().tolist() == idx                       # per-row class ids and each group's vote
    assert gcpp.feature.shape[0] == 2 * N and gcpp.gradient.shape[0] == 2 * N
    for (ms, gs), mp, gp in zip(sep, (m1, m2), (g1, g2)):
        assert mp.shape == (N, 1, H, W) and gp.shape == (N, 3, H, W)
        assert float((mp - ms).abs().max()) < 2e-3
        assert float((gp - gs).abs().max()) < 3e-3 * float(gs.abs().max())
    # one conv sequence for both batches: the ops of ONE separate pass on 2N rows, and ONE separate pass's KERNEL_LOG with the
    # group forms in place of the batch forms
    assert logs[0] == logs[1]
    names1, calls1 = logs[0]
    assert [c[0] for c in calls1].count("conv2d") == 26          # 13 forward + 13 data-gradient convs
    assert calls == [(op, (2 * N,) + shp[1:]) for op, shp in calls1]
    assert "class_target" in names1 and names.count("class_target_groups") == 1 and names.count("gather_row_groups") == 1
    assert [n for n in names if n != "gather_row_groups"] == [n.replace("class_target", "class_target_groups") for n in names1]
    # classes given per row: each half keeps its own vote (here 3 against 7), which a vote over all 2N rows would not
    ids = [3] * N + [7] * N
    mp1, gp1, mp2, gp2 = gcpp.with_input_gradient_pair(imgs1, imgs2, index=ids)
    assert [r[0] for r in gcpp.index.cpu().tolist()] == [3, 7]
    for imgs, sl, mp, gp in ((imgs1, slice(0, N), mp1, gp1), (imgs2, slice(N, 2 * N), mp2, gp2)):
        ms, gs = gcpp.with_input_gradient(imgs, index=ids[sl])
        assert float((mp - ms).abs().max()) < 2e-3
        assert float((gp - gs).abs().max()) < 3e-3 * float(gs.abs().max())
    with pytest.raises(ValueError):
        gcpp.with_input_gradient_pair(imgs1, imgs2[:1])


def test_calls_without_the_new_keywords_issue_the_launches_they_issued_before():
    G, net = _net()
    gcpp = G.GradCamPlusPlus(net, net.final_layer)
    G.GuidedBackPropagation(net)
    imgs = R.gradcam_images("a", 2, 32, 32).cuda()
    lg = net(imgs)
    _, names, _ = _logged(lambda: net.select_target(lg))
    assert names == ["class_target"]
    mask, names, _ = _logged(lambda: gcpp(imgs, None))
    assert "class_target" in names and not any("groups" in n for n in names)
    _, names, _ = _logged(lambda: G.mask2cam(mask, imgs))
    assert names == ["mask2cam"]
    _, names, _ = _logged(lambda: G.mask2cam(mask, imgs, rows=True))
    assert names == ["mask2cam_rows"]
