"""dge_amd.noise_maps.NoiseMaps, the owner of the optimised noise maps that LatentEmbedStep and ProjectorStep share, on the small
synthesis of tests/s2_noise_models.py (maps of 4^2 ... 64^2) with one shared set of maps and with a set per row: every method
against the expression or the direct ops call it stands for, to the bit."""
import pytest
import torch

from tests.s2_noise_models import S2N_KW, S2N_RES, s2n_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def synthesis():
    import dge_amd
    G = dge_amd.StyleGAN2Generator(64, compute_dtype="f32", **S2N_KW).cuda()
    G.load_state_dict(s2n_state_dict())
    G.eval()
    return G.synthesis


@pytest.mark.parametrize("Bn", [1, 2])
def test_noise_maps_methods_are_the_direct_calls(synthesis, Bn):
    from dge_amd import ops
    from dge_amd.noise_maps import NoiseMaps
    dev = torch.device("cuda", torch.cuda.current_device())
    nm = NoiseMaps(synthesis, Bn, dev)
    assert [tuple(m.shape) for m in nm.maps] == [(Bn, r, r) for r in S2N_RES] == [tuple(g.shape) for g in nm.grads]
    assert nm.flat.requires_grad and all(m.requires_grad for m in nm.maps) and tuple(nm.reg.shape) == (Bn,)
    assert nm.fits(Bn, dev) and not nm.fits(Bn + 1, dev) and not nm.fits(Bn, "cpu")

    # reset(): every row of every map is the generator's buffer, in place
    ptr = nm.flat.data_ptr()
    for _ in range(2):
        nm.flat.detach().fill_(3.0)
        nm.reset()
        assert nm.flat.data_ptr() == ptr
        for i, m in enumerate(nm.maps):
            buf = getattr(synthesis, f"layer{i}").noise.reshape(S2N_RES[i], S2N_RES[i])
            assert m.data_ptr() == nm.table.view(nm.flat.detach(), i).data_ptr()
            assert all(torch.equal(m[b].detach(), buf) for b in range(Bn)), i
    assert all(torch.equal(a, b.detach()) for a, b in zip(nm.detached(), nm.maps)) and not any(a.requires_grad for a in nm.detached())

    # add_reg / normalize on maps that differ from row to row and a gradient buffer that is not empty (the regulariser ACCUMULATES)
    gen = torch.Generator().manual_seed(5)
    nm.flat.detach().copy_(torch.randn(nm.table.numel, generator=gen))
    nm.gflat.copy_(torch.randn(nm.table.numel, generator=gen))
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        flat, grad, out = nm.flat.detach().clone(), nm.gflat.clone(), torch.full((Bn,), -1.0, device=dev)
        ops.noise_reg(nm.table, flat, grad=grad, scale=1e5, accumulate=True, out=out)
        reg = nm.add_reg(1e5)
        assert reg is nm.reg and torch.equal(reg, out) and torch.equal(nm.gflat, grad) and torch.equal(nm.flat.detach(), flat)
        assert float(reg.min()) > 0.0 and not torch.equal(nm.grads[-1], torch.zeros_like(nm.grads[-1]))
        nm.hand_grad()
        assert nm.flat.grad is nm.gflat
        ops.noise_normalize(nm.table, flat)
        nm.normalize()
        assert torch.equal(nm.flat.detach(), flat) and nm.flat.data_ptr() == ptr
        assert all(abs(float(m.detach().double().pow(2).mean()) - 1.0) < 1e-5 for m in nm.maps)          # (it did normalise)
    finally:
        ops.set_deterministic(was)
