"""Pins tests/golden/encpg_imggrad.npz (tools/gen_golden_embed_pg.py: the reference E_PG.BE with the input image requiring a
gradient) on the oracle's E_PG under torch autograd: the loss and g_img within the bounds
test_encvar.test_oracle_e_pg_gradients_vs_reference_golden sets for the parameter gradients (loss 1e-4, gradients 2e-3)."""
import torch

from tests.conftest import golden, with_fixture_params
from tests.golden import recipe as R
from tests.test_encvar import _l2rel, pg_params
from oracle import ref_torch as O


def test_oracle_e_pg_image_gradient_vs_reference_golden():
    from dge_amd.encoder_variants import PGBE
    g0, g = golden("encpg_small.npz"), golden("encpg_imggrad.npz")
    P = {k: v.clone().requires_grad_(True) for k, v in with_fixture_params(pg_params(PGBE(startf=32, maxf=512, layer_count=5, pggan=True)), g).items()}
    noises = [R.randn(f"ep.noise{i}", tuple(s), 62) for i, s in enumerate(g0["noise_shapes"].tolist())]
    img = R.randn("ep.img", (2, 3, 64, 64), 62, 0.5).requires_grad_(True)
    _, z = O.encpg_forward(P, img, noises, 5)
    loss = (z * R.randn("ep.gz", tuple(z.shape), 64)).sum()
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    assert img.grad.shape == (2, 3, 64, 64) and float(torch.as_tensor(g["g_img"]).norm()) > 0
    assert _l2rel(img.grad, g["g_img"]) < 2e-3
    assert _l2rel(z, g["z"]) < 2e-4


def test_fixture_agrees_with_the_parameter_gradient_fixture():
    """The image gradient changes nothing else: same nudged parameters, loss and (first 4096 entries of the) parameter gradients as
    encpg_grad.npz, which stores larger slices."""
    g, gp = golden("encpg_imggrad.npz"), golden("encpg_grad.npz")
    assert float(g["loss"]) == float(gp["loss"]) and float(g["kink_margin"]) == float(gp["kink_margin"])
    keys = [k for k in g.files if k.startswith(("param:", "norm:"))]
    assert keys and sorted(keys) == sorted(k for k in gp.files if k.startswith(("param:", "norm:")))
    for k in keys:
        assert (g[k] == gp[k]).all(), k
    for k in (k for k in g.files if k.startswith("grad:")):
        assert (g[k].reshape(-1)[:4096] == gp[k].reshape(-1)[:4096]).all(), k
