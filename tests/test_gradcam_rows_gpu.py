"""The per-row attention pieces (grad_cam.GradCAM.call_per_image, mask2cam(rows=True), VGG16.select_target_rows) against the
reference's own GradCamPlusPlus.call_per_image / one-row mask2cam (tests/golden/gradcam_rows.npz, tools/gen_golden_embed_big_rows.py)
and against the coupled calls on the one-row slices.  B = 3, K = 40 classes (no multiple of the 64-lane wave).  The fixture's images
make the coupled forms differ: the rows' arg-max classes are not all equal, and a later row holds the batch's minimum."""
import functools

import numpy as np
import pytest
import torch

from tests.conftest import golden
from tests.golden import recipe as R
from tests.test_gradcam import CFG, _net

pytestmark = pytest.mark.gpu
MASK_TOL, CAM_TOL = 2e-3, 1e-2          # tests/test_gradcam.py: the coupled forms against gradcam.npz


def _imgs(g):
    scale = torch.as_tensor(g["img_scale"]).view(-1, 1, 1, 1)
    return (R.gradcam_images(str(g["img_tag"]), 3, CFG["H"], CFG["W"]) * scale).cuda()


def _guided_gcpp():
    G, net = _net("f32")
    gcpp = G.GradCamPlusPlus(net, net.final_layer)
    G.GuidedBackPropagation(net)            # the fixture's wiring: one shared network, every backward the guided one
    return G, net, gcpp


def _traced(fn):
    from dge_amd import ops
    ops.KERNEL_LOG = log = []
    try:
        out = fn()
    finally:
        ops.KERNEL_LOG = None
    return out, [n for n, _ in log]


def _check_cam(heat, cam, ref_heat, ref_cam, where):
    # the JET index is uint8(255 * mask) by truncation: a pixel within rounding of an integer may take the neighbouring entry
    dh = np.abs(heat.cpu().numpy() - ref_heat)
    assert dh.max() <= 4.0 / 255 + 1e-6 and (dh > 1e-6).mean() < 1e-3, (where, dh.max())
    dc = np.abs(cam.cpu().numpy() - ref_cam)
    print("MEAS gradcam_rows cam", where, float(dc.max()))
    assert dc.max() < CAM_TOL and (dc > 1e-5).mean() < 1e-3, (where, dc.max())


def test_call_per_image_and_mask2cam_rows_vs_reference_run():
    g = golden("gradcam_rows.npz")
    assert len(set(g["index"].tolist())) > 1 and float(g["mask_coupled_diff"].max()) > 10 * MASK_TOL \
        and float(g["cam_coupled_diff"].max()) > 10 * CAM_TOL          # what the generator asserted
    G, net, gcpp = _guided_gcpp()
    imgs = _imgs(g)
    logits = net(imgs).cpu().numpy()
    assert np.abs(logits - g["logits"]).max() < 2e-4 * np.abs(g["logits"]).max()
    mask, names = _traced(lambda: gcpp.call_per_image(imgs, None))
    assert "class_target_rows" in names and "gather_rows" in names and "class_target" not in names
    assert gcpp.index.cpu().tolist() == g["index"].tolist()
    assert mask.shape == (3, 1, CFG["H"], CFG["W"]) and mask.dtype == torch.float32 and mask.is_cuda
    dm = np.abs(mask.cpu().numpy() - g["mask_rows"]).reshape(3, -1).max(1)
    print("MEAS gradcam_rows mask", dm.tolist())
    assert dm.max() < MASK_TOL, dm
    # mask2cam on the reference's masks (isolates it from the network)
    (heat, cam), names = _traced(lambda: G.mask2cam(torch.from_numpy(g["mask_rows"]).cuda(), imgs, rows=True))
    assert names == ["mask2cam_rows"]
    _check_cam(heat, cam, g["heat_rows"], g["cam_rows"], "golden")


def test_rows_equal_the_coupled_calls_on_one_row_slices_and_not_the_coupled_batch():
    g = golden("gradcam_rows.npz")
    G, net, gcpp = _guided_gcpp()
    imgs = _imgs(g)
    mask = gcpp.call_per_image(imgs, None)
    ref_mask = torch.from_numpy(g["mask_rows"]).cuda()
    heat, cam = G.mask2cam(ref_mask, imgs, rows=True)
    for b in range(3):
        one, names = _traced(lambda: gcpp(imgs[b:b + 1], None))
        assert "class_target" in names and "class_target_rows" not in names
        assert float((mask[b:b + 1] - one).abs().max()) < MASK_TOL, b
        (h1, c1), names = _traced(lambda: G.mask2cam(ref_mask[b:b + 1], imgs[b:b + 1]))
        assert names == ["mask2cam"]
        _check_cam(heat[b:b + 1], cam[b:b + 1], h1.cpu().numpy(), c1.cpu().numpy(), b)
    # the coupled B = 3 calls are other computations: the reference's own differ by > 10x the tolerance on the rows the fixture names,
    # and each HIP form lies within 1x of its reference
    rm, rc = int(g["mask_diff_row"]), int(g["cam_diff_row"])
    d_mask = float((gcpp(imgs, None)[rm] - mask[rm]).abs().max())
    d_cam = float((G.mask2cam(ref_mask, imgs)[1][rc] - cam[rc]).abs().max())
    print("MEAS gradcam_rows coupled", d_mask, d_cam)
    assert d_mask > 8 * MASK_TOL and d_cam > 8 * CAM_TOL, (d_mask, d_cam)


@functools.lru_cache(maxsize=None)
def _logits():
    """[5, 130]: ties inside one lane (3 and 67), across lanes and strides (7, 70, 129), in neighbouring lanes of the second stride
    (64, 65), a maximum in the 2-wide tail past 128, and a constant row."""
    x = R.randn("gradcam_rows.logits", (5, 130), 0).clamp(-3, 3)
    x[0, [7, 70, 129]] = 5.0
    x[1, 129] = 4.0
    x[2, [64, 65]] = 6.0
    x[3, [67, 3]] = 4.5
    x[4, :] = -1.25
    return x


def test_select_target_rows_first_maximum_given_index_and_one_hot():
    from dge_amd import grad_cam
    net = grad_cam.VGG16(CFG["widths"], CFG["fc"], CFG["classes"])
    x = _logits()
    want = x.numpy().argmax(1)
    assert want.tolist() == [7, 129, 64, 3, 0]
    idx, gl = net.select_target_rows(x.cuda(), None)
    assert idx.dtype == torch.int32 and idx.cpu().tolist() == want.tolist()
    assert torch.equal(gl.cpu(), torch.nn.functional.one_hot(torch.as_tensor(want), 130).float())
    given = [1, 129, 64, 0, 77]
    for index in (given, np.array(given), torch.tensor(given).cuda()):
        idx, gl = net.select_target_rows(x.cuda(), index)
        assert idx.cpu().tolist() == given
        assert torch.equal(gl.cpu(), torch.nn.functional.one_hot(torch.as_tensor(given), 130).float())
    # the gather of rows that starts the per-row backward: y[b, :] = w[index[b], :], exactly (I = 37: no multiple of anything)
    from dge_amd import ops
    from dge_amd._lib import check, lib
    w = R.randn("gradcam_rows.w6", (130, 37), 0).cuda()
    y = torch.empty((5, 37), dtype=torch.float32, device="cuda")
    check(lib().dge_gather_rows(ops._f32(w), ops._p(idx), ops._f32(y), 5, 37, ops._stream()), "dge_gather_rows")
    assert torch.equal(y, w[torch.tensor(given).cuda()])
    with pytest.raises(ValueError):
        net.select_target_rows(x.cuda(), [0, 1, 2, 3, 130])
    with pytest.raises(ValueError):
        net.select_target_rows(x.cuda(), [0, 1, 2])


def test_rows_forms_give_the_same_bits_run_to_run_in_both_reduction_modes():
    from dge_amd import ops
    g = golden("gradcam_rows.npz")
    G, net, gcpp = _guided_gcpp()
    imgs = _imgs(g)
    ref_mask = torch.from_numpy(g["mask_rows"]).cuda()
    x = _logits().cuda()
    was = ops.is_deterministic()
    res = []
    try:
        for det in (False, True, False, True):
            ops.set_deterministic(det)
            idx, gl = net.select_target_rows(x, None)
            heat, cam = G.mask2cam(ref_mask, imgs, rows=True)
            res.append((idx.clone(), gl.clone(), gcpp.call_per_image(imgs, None).clone(), heat, cam))
    finally:
        ops.set_deterministic(was)
    for other in res[1:]:          # the new kernels: no atomics and no mode-dependent path
        for k in (0, 1, 3, 4):
            assert torch.equal(res[0][k], other[k]), k
    # the whole per-image mask (the network's convolutions may take another kernel in the other mode): run to run within a mode
    assert torch.equal(res[0][2], res[2][2]) and torch.equal(res[1][2], res[3][2])
