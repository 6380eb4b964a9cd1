"""E.BE's hand-written backward beyond E_align's case: gradients through the const output and to the input image, with the encoder
trained or frozen (what embedding_v2 back-propagates through E(imgs2)), against the reference's autograd
(tests/golden/enc_small.npz: a loss on w; tests/golden/enc_be_grad.npz: a loss on both outputs)."""
import numpy as np
import pytest
import torch

from tests.conftest import MODES, golden, meas, with_fixture_params
from tests.golden import recipe as R
from tests.helpers import enc_shapes
from oracle import ref_torch as O

pytestmark = pytest.mark.gpu


def l2rel(a, b):
    a = a.detach().float().cpu().flatten(); b = torch.as_tensor(np.asarray(b)).float().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def be_encoder(cd, L=5, seed=81, fixture="enc_be_grad.npz"):
    from dge_amd.encoder import BE
    E = BE(startf=16, maxf=64, layer_count=L, compute_dtype=cd).cuda()
    E.load_state_dict(with_fixture_params(R.fill_encoder(enc_shapes(16, 64, L), seed=seed), golden(fixture)))
    return E


def be_inputs():
    img = R.randn("ebe.img", (2, 3, 64, 64), 81, 0.5).cuda()
    noises = [R.randn(f"ebe.noise{i}", s, 81).cuda() for i, s in enumerate(O.enc_noise_shapes(5, 2, 64))]
    return img, noises


def param_grad_errors(E, g):
    """Relative L2 per parameter gradient against the fixture's entries (the first 4096 elements of a large tensor, and its norm);
    a parameter without an entry must have no gradient."""
    errs = {}
    for k, p in E.named_parameters():
        if "grad:" + k not in g.files:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        nrm = float(g["norm:" + k])
        if nrm < 1e-3:      # conv_3.bias in front of an instance norm: the true gradient is zero, the reference holds rounding noise
            assert float(p.grad.norm()) < 5e-2, (k, float(p.grad.norm()))
            continue
        mine = p.grad.detach().float().cpu()
        errs[k] = max(l2rel(mine if mine.numel() <= 4096 else mine.flatten()[:4096], g["grad:" + k]), abs(float(mine.norm()) - nrm) / nrm)
    assert len(errs) >= 40, len(errs)
    return errs


def test_hip_e_be_image_gradient_vs_reference_golden_small():
    """E_align's loss (on w only) with the image requiring a gradient, f32: the image gradient the reference's autograd gives
    (enc_small.npz `grad_img`, read by no other GPU test) and the parameter gradients as tests/test_enc_gpu.py checks them."""
    from tests.test_enc_gpu import small_encoder
    g = golden("enc_small.npz")
    E = small_encoder("f32")
    img = R.randn("enc.img", (2, 3, 32, 32), 9, 0.5).cuda().requires_grad_(True)
    noises = [R.randn(f"enc.noise{i}", s, 9).cuda() for i, s in enumerate(O.enc_noise_shapes(4, 2, 32))]
    x, w = E(img, noises=noises)
    (w * R.randn("enc.gw", tuple(w.shape), 9, 0.05).cuda()).sum().backward()
    e_img = l2rel(img.grad, g["grad_img"])
    worst = 0.0
    for k, p in E.named_parameters():
        if "grad:" + k in g.files:
            a, b = p.grad.float().cpu().flatten(), torch.from_numpy(g["grad:" + k]).flatten()
            worst = max(worst, ((a - b).abs().max() / b.abs().max()).item())
        else:
            assert p.grad is None, k
    meas("enc_be_small_img_grad", img_l2=e_img, worst_param_maxrel=worst)
    assert e_img < 1e-3, e_img          # the project's f32 gradient bound (E_Blur's image gradient measured 1.7e-4)
    assert worst < 1e-4, worst          # test_encoder_backward_vs_reference_golden's deterministic f32 bound


# bf16 on the 64^2 fixture, relative L2 against the golden as measured on an MI355X: deterministic run - image gradient 0.144, worst
# parameter tensor 0.197 (decode_block.0.noise_weight_2: a sum of g * noise over 2 x 64^2 pixels with heavy cancellation, of
# bf16-stored operands); default (atomics) run - 0.142 and 0.164 (decode_block.1.noise_weight_2).  Bounds = 1.5x the values of the
# run, never above E_Blur's (0.43 on its image gradient, 0.48 per tensor: tests/test_encvar.py).  The f32 runs are the parity check
# of the formulas.
BF16_MEASURED = {"det": dict(img=0.1441, worst=0.1965), "atomics": dict(img=0.1419, worst=0.1643)}
BF16_CAP = dict(img=0.43, worst=0.48)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_hip_e_be_gradients_vs_reference_golden(cd, mode):
    """A loss on BOTH outputs, image requiring a gradient: g_img and every parameter gradient against the reference's autograd; a
    const-only and a w-only loss each reach the image."""
    g = golden("enc_be_grad.npz")
    E = be_encoder(cd)
    img0, noises = be_inputs()
    img = img0.clone().requires_grad_(True)
    x, w = E(img, noises=noises)
    gx, gw = R.randn("ebe.gx", tuple(x.shape), 83).cuda(), R.randn("ebe.gw", tuple(w.shape), 83).cuda()
    loss = (x * gx).sum() + (w * gw).sum()
    loss.backward()
    e_img = l2rel(img.grad, g["g_img"])
    errs = param_grad_errors(E, g)
    wk = max(errs, key=errs.get)
    meas("enc_be_grads", cd=cd, mode=mode, img_l2=e_img, worst_l2=errs[wk], key=wk, x_l2=l2rel(x, g["x"]), w_l2=l2rel(w, g["w"]),
         loss_rel=abs(float(loss.detach()) - float(g["loss"])) / abs(float(g["loss"])))
    if cd == "f32":
        assert e_img < 1e-3, e_img
        assert errs[wk] < 1e-3, (wk, errs[wk])
    else:
        for name, val in (("img", e_img), ("worst", errs[wk])):
            assert val < min(1.5 * BF16_MEASURED[mode][name], BF16_CAP[name]), (name, val)
    for which in ("const", "w"):
        im = img0.clone().requires_grad_(True)
        x, w = E(im, noises=noises)
        ((x * gx).sum() if which == "const" else (w * gw).sum()).backward()
        assert torch.isfinite(im.grad).all() and float(im.grad.abs().max()) > 0.0, which


def test_frozen_e_be_backward_computes_the_data_gradient_only(monkeypatch):
    """Mirrors test_embed_v2_gpu.py::test_frozen_encoder_backward_computes_the_data_gradient_only for E.BE."""
    from dge_amd import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        img0, noises = be_inputs()
        gw = R.randn("ebe.gw", (2, 10, 512), 83).cuda()
        gc = R.randn("ebe.gx", (2, 64, 4, 4), 83).cuda()

        def img_grad(E):
            x = img0.clone().requires_grad_(True)
            c, w = E(x, noises=noises)
            torch.autograd.backward([c, w], [gc, gw])
            return x.grad.clone()
        Et = be_encoder("bf16")
        g_train = img_grad(Et)
        assert all((p.grad is not None) == ("grad:" + k in golden("enc_be_grad.npz").files) for k, p in Et.named_parameters())
        Ef = be_encoder("bf16")
        for p in Ef.parameters():
            p.requires_grad_(False)

        def boom(*a, **kw):
            raise AssertionError("weight-gradient kernel called with a frozen encoder")
        for name in ("conv_wgrad", "conv_wgrad_dots", "fromrgb_bwd", "dense_wgrad"):
            monkeypatch.setattr(ops, name, boom)
        g_frozen = img_grad(Ef)
        assert torch.isfinite(g_frozen).all() and float(g_frozen.abs().max()) > 0.0
        assert torch.equal(g_frozen, g_train)
        assert all(p.grad is None for p in Ef.parameters())
    finally:
        ops.set_deterministic(was)


def test_e_align_style_backward_is_unchanged(monkeypatch):
    """Image detached, loss on w (E_align): the backward never reaches the image-gradient launch, and its parameter gradients are
    the same bits with that launch made unavailable."""
    from dge_amd import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        img0, noises = be_inputs()
        gw = R.randn("ebe.gw", (2, 10, 512), 83).cuda()

        def run():
            E = be_encoder("bf16")
            x, w = E(img0, noises=noises)
            (w * gw).sum().backward()
            return {k: p.grad.clone() for k, p in E.named_parameters() if p.grad is not None}
        a = run()

        def boom(*args, **kw):
            raise AssertionError("in_bwd_fromrgb_img launched without an image gradient to compute")
        monkeypatch.setattr(ops, "in_bwd_fromrgb_img", boom)
        b = run()
        assert a.keys() == b.keys() and len(a) >= 40
        for k in a:
            assert torch.equal(a[k], b[k]), k
    finally:
        ops.set_deterministic(was)
