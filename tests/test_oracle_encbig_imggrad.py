"""Pins tests/golden/encbig_imggrad.npz on the CPU: autograd through the oracle's restatement of E_BIG (train mode: one spectral-norm
power iteration, gradient through sigma) w.r.t. the input image and every parameter reproduces the reference's own gradients."""
import numpy as np
import torch

from tests.conftest import golden, with_fixture_params
from tests.golden import recipe as R
from oracle import ref_torch as O


def _l2rel(a, b):
    a = a.detach().float().flatten(); b = torch.as_tensor(np.asarray(b)).float().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def test_oracle_e_big_image_gradient_vs_reference_golden():
    from dge_amd.encoder_variants import BigBE
    g0, g = golden("encbig_small.npz"), golden("encbig_imggrad.npz")
    E = BigBE(startf=32, maxf=512, layer_count=5, biggan=True)
    P = with_fixture_params(R.fill_encbig({n: list(v.shape) for n, v in E.state_dict().items()}, 81), g)
    O.bg_sn_power_iteration(P, eps=1e-12)
    P = {k: (v.clone().requires_grad_(True) if (v.dtype.is_floating_point and "running_" not in k and "weight_u" not in k and "weight_v" not in k) else v)
         for k, v in P.items()}
    noises = [R.randn(f"ebg.noise{i}", tuple(s), 81) for i, s in enumerate(g0["noise_shapes"].tolist())]
    img = R.randn("ebg.img", (2, 3, 64, 64), 81, 0.5).requires_grad_(True)
    _, c_v, z = O.encbig_forward(P, img, R.randn("ebg.cond", (2, 256), 81, 0.5), noises, 5)
    loss = (z * R.randn("ebg.gz", tuple(z.shape), 82)).sum() + (c_v * R.randn("ebg.gcv", tuple(c_v.shape), 82)).sum()
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    # the bound of test_encvar.test_oracle_e_big_gradients_vs_reference_golden
    tol = 2e-3
    assert tuple(g["g_img"].shape) == (2, 3, 64, 64)
    assert _l2rel(img.grad, g["g_img"]) < tol, _l2rel(img.grad, g["g_img"])
    checked = 0
    for k, v in P.items():
        if not v.requires_grad or "grad:" + k not in g.files:
            continue
        nrm = float(g["norm:" + k])
        if nrm < 1e-3:
            continue
        mine = v.grad.detach().float()
        assert abs(float(mine.norm()) - nrm) < tol * nrm + 1e-6, k
        assert _l2rel(mine if mine.numel() <= 4096 else mine.flatten()[:4096], g["grad:" + k]) < tol, k
        checked += 1
    assert checked >= 60, checked
