"""The float64 restatement of the noise regulariser the GPU tests compare with (tests/s2_noise_models.py: explicit 2x2 means and
wrapped neighbours, the closed-form gradient of the README) against the fixture's values and gradients, which
tools/gen_golden_s2_noise.py computed as StyleGAN2's projector does (avg_pool2d, torch.roll, autograd)."""
import torch

from tests.conftest import golden
from tests.golden import recipe as R
from tests.s2_noise_models import levels, normalize_ref, reg_grad_ref, reg_ref


def test_restatement_reproduces_the_fixture():
    g = golden("s2_noise_grad.npz")
    for r in (4, 8, 16, 64):
        n = R.randn(f"s2n.reg{r}", (3, r, r), 9, 1.3, 0.2).double()
        want, want_g = torch.as_tensor(g[f"reg{r}"]), torch.as_tensor(g[f"reg_grad{r}"])
        assert want.dtype == torch.float64
        got = reg_ref(n)
        assert ((got - want).abs() / want.abs()).max().item() < 1e-12, r
        leaf = n.clone().requires_grad_(True)
        reg_ref(leaf).sum().backward()
        for gg in (leaf.grad, reg_grad_ref(n)):          # autograd of the restatement, and the closed form
            assert ((gg - want_g).abs().max() / want_g.abs().max()).item() < 1e-12, r


def test_levels_and_normalisation():
    assert [levels(r) for r in (4, 8, 16, 32, 64, 256, 512, 1024)] == [1, 1, 2, 3, 4, 6, 7, 8]
    n = normalize_ref(R.randn("s2n.norm", (2, 16, 16), 3, 1.7, -0.4))
    assert n.mean(dim=(1, 2)).abs().max().item() < 1e-14 and ((n * n).mean(dim=(1, 2)) - 1).abs().max().item() < 1e-14


def test_ops_table_layout_matches_the_restatement():
    """ops.noise_levels (what the device table is built from) agrees with the restatement's pyramid."""
    from dge_amd import ops
    assert all(ops.noise_levels(r) == levels(r) for r in (4, 8, 16, 32, 64, 128, 256, 512, 1024))
