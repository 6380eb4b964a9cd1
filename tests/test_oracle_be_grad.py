"""The oracle's E.BE (oracle.ref_torch.enc_forward, differentiated by autograd) against the reference's own gradients for a loss on
BOTH encoder outputs, parameters and input image (tests/golden/enc_be_grad.npz, tools/gen_golden.py `encgrad_be`)."""
import torch

from tests.conftest import golden, with_fixture_params
from tests.golden import recipe as R
from tests.helpers import enc_shapes
from oracle import ref_torch as O


def _l2rel(a, b):
    a, b = a.detach().double().flatten(), torch.as_tensor(b).double().flatten()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def test_oracle_e_be_gradients_vs_reference_golden():
    g = golden("enc_be_grad.npz")
    P = {k: v.clone().requires_grad_(True) for k, v in with_fixture_params(R.fill_encoder(enc_shapes(16, 64, 5), seed=81), g).items()}
    shp = O.enc_noise_shapes(5, 2, 64)
    assert [list(s) for s in shp] == g["noise_shapes"].tolist()
    noises = [R.randn(f"ebe.noise{i}", s, 81) for i, s in enumerate(shp)]
    img = R.randn("ebe.img", (2, 3, 64, 64), 81, 0.5).requires_grad_(True)
    x, w = O.enc_forward(P, img, noises)
    loss = (x * R.randn("ebe.gx", tuple(x.shape), 83)).sum() + (w * R.randn("ebe.gw", tuple(w.shape), 83)).sum()
    loss.backward()
    assert _l2rel(x, g["x"]) < 1e-4 and _l2rel(w, g["w"]) < 1e-4
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    assert _l2rel(img.grad, g["g_img"]) < 1e-4, _l2rel(img.grad, g["g_img"])        # (measured 1.4e-6)
    checked = 0
    for k, p in P.items():
        if "grad:" + k not in g.files:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        nrm = float(g["norm:" + k])
        if nrm < 1e-3:       # conv_3.bias in front of an instance norm: the true gradient is zero, the reference holds rounding noise
            assert float(p.grad.norm()) < 1e-3, k
            continue
        assert abs(float(p.grad.norm()) - nrm) < 1e-4 * nrm, k
        mine = p.grad if p.grad.numel() <= 4096 else p.grad.flatten()[:4096]
        assert _l2rel(mine, g["grad:" + k]) < 1e-4, (k, _l2rel(mine, g["grad:" + k]))
        checked += 1
    assert checked >= 40, checked
