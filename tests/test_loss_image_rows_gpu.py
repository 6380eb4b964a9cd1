"""losses.space_loss_image_rows: the per-sample space_loss on one full window with LPIPS, for images [B,3,H,W] and maps [B,1,H,W] -
row b against the coupled losses.space_loss on the one-row slices, in value and in gradient.  B = 3 at 32 x 32; the rows of the second
argument are scaled differently (as in tests/test_loss_rows_gpu.py), so the per-sample losses lie far apart.  Bounds: those
test_loss_rows_gpu.py applies to a rows form against the coupled form on one-row slices (value 2e-4, logged terms 5e-4 + 2e-6,
gradient 2e-3 of its largest element)."""
import functools

import pytest
import torch

from tests.golden import recipe as R
from tests.test_loss_rows_gpu import _check_info, _scaled_rows
from oracle import lpips_ref as LR

pytestmark = pytest.mark.gpu
B, S = 3, 32


@functools.lru_cache(maxsize=None)
def _lpips():
    from dge_amd.lpips import LPIPS
    LP = LPIPS(compute_dtype="f32").cuda()
    LP.load_state_dict(LR.seeded_params(0))
    return LP


def _pair(ch):
    a = torch.tanh(R.randn(f"imgrows.a{ch}", (B, ch, S, S), 3, 0.6))
    b = _scaled_rows(a, R.randn(f"imgrows.b{ch}", (B, ch, S, S), 3, 0.2)).clamp(-1, 1)
    return a.cuda(), b.cuda()


def _compare(a, b, lp_rows, lp_one, grad):
    """rows form with `lp_rows` against space_loss on every one-row slice with `lp_one`; `grad`: with the gradient of both."""
    from dge_amd import losses
    ctx = torch.enable_grad() if grad else torch.no_grad()
    with ctx:
        bg = b.clone().requires_grad_(grad)
        loss, info = losses.space_loss_image_rows(a, bg, lpips_model=lp_rows)
        if grad:
            loss.backward()
        assert tuple(info.shape) == (B, 8)
        tot = 0.0
        for r in range(B):
            y = b[r:r + 1].clone().requires_grad_(grad)
            l, i8 = losses.space_loss(a[r:r + 1], y, lpips_model=lp_one)
            tot += float(l)
            e_l = abs(float(info[r, 0]) - float(l)) / abs(float(l))
            print("MEAS image_rows", tuple(a.shape), r, float(info[r, 0]), float(l), e_l)
            assert e_l < 2e-4, (r, float(info[r, 0]), float(l))
            _check_info(info[r].cpu(), i8.cpu(), r)
            if grad:
                l.backward()
                e_g = ((bg.grad[r:r + 1] - y.grad).abs().max() / y.grad.abs().max()).item()
                print("MEAS image_rows grad", r, e_g)
                assert e_g < 2e-3, (r, e_g)
        assert abs(float(loss) - tot) < 2e-4 * tot
    assert abs(float(info[0, 0]) - float(info[2, 0])) > 0.1 * float(info[0, 0])          # the rows are told apart
    return info


def test_image_rows_three_channels_value_and_gradient_equal_one_row_slices():
    a, b = _pair(3)
    info = _compare(a, b, _lpips(), _lpips(), grad=True)
    assert float(info[:, 7].min()) > 0.0          # LPIPS took part


def test_image_rows_one_channel_value_and_gradient_equal_one_row_slices():
    """The Grad-CAM masks: LPIPS feeds a one-channel map as three equal channels and offers no gradient for it (the loops use these
    terms as values) - the value is compared with LPIPS, the gradient of the remaining terms without it."""
    a, b = _pair(1)
    info = _compare(a, b, _lpips(), _lpips(), grad=False)
    assert float(info[:, 7].min()) > 0.0
    _compare(a, b, None, None, grad=True)


def test_image_rows_refusals_stay():
    from dge_amd import losses
    a, b = _pair(3)
    with pytest.raises(ValueError):
        losses.space_loss_rows(a, b, image_space=True)
    with pytest.raises(ValueError):
        losses.space_loss_image_rows(a, b, global_batch=losses.GlobalBatch(2))
    with pytest.raises(ValueError):
        losses.space_loss_image_rows(a.view(B, -1), b.view(B, -1))
