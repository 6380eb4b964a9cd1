"""StyleGAN2Generator.synthesis(wp, noises=...): the conv layers' noise maps as differentiable inputs.  The model is the 64^2
generator of tests/s2_noise_models.py (every noise strength at magnitude about 0.1); the gradients are compared with the
reference's autograd (tests/golden/s2_noise_grad.npz, tools/gen_golden_s2_noise.py) inside the grad_wp bound of
tests/test_s2_gpu.py::test_synthesis_grad_wp_vs_reference_golden, as relative L2."""
import pytest
import torch

from tests.conftest import MODES, golden, meas, with_fixture_params
from tests.golden import recipe as R
from tests.s2_noise_models import S2N_KW, S2N_RES, s2n_state_dict
from tests.test_embed_v2_gpu import l2rel

pytestmark = pytest.mark.gpu
NL = len(S2N_RES)


def generator(cd):
    import dge_amd
    G = dge_amd.StyleGAN2Generator(64, compute_dtype=cd, **S2N_KW).cuda()
    # (the fixture's conv biases: moved off the leaky-relu kink for its three forwards, tools/gen_golden.py clear_kinks)
    G.load_state_dict(with_fixture_params(s2n_state_dict(), golden("s2_noise_grad.npz")))
    G.eval()
    for p in G.parameters():
        p.requires_grad_(False)
    return G


def buffers(G, B=1):
    return [getattr(G.synthesis, f"layer{i}").noise.detach().reshape(1, r, r).expand(B, r, r).contiguous() for i, r in enumerate(S2N_RES)]


def row_maps(B=2):
    return [R.randn(f"s2n.noise{i}", (2, r, r), 7)[:B].cuda() for i, r in enumerate(S2N_RES)]


def wp_gimg():
    wp = R.randn("s2n.wp", (2, 10, 512), 5).cuda()
    return wp, R.randn("s2n.gimg", (2, 3, 64, 64), 5, 1.0 / (2 * 3 * 64 * 64) ** 0.5).cuda()


@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_noises_equal_to_the_buffers_give_the_default_image_to_the_bit(cd):
    G = generator(cd)
    wp, _ = wp_gimg()
    with torch.no_grad():
        ref = G.synthesis(wp)["image"]
        assert torch.equal(G.synthesis(wp, noises=buffers(G))["image"], ref)
        assert torch.equal(G.synthesis(wp, noises=buffers(G, 2))["image"], ref)          # a copy per row
    leaves = [n.requires_grad_(True) for n in buffers(G)]
    assert torch.equal(G.synthesis(wp, noises=leaves)["image"].detach(), ref)          # (the saving forward)
    with pytest.raises(ValueError, match="randomize_noise"):
        G.synthesis(wp, randomize_noise=True, noises=buffers(G))
    with pytest.raises(ValueError, match="one map per conv layer"):
        G.synthesis(wp, noises=buffers(G)[:-1])
    with pytest.raises(ValueError, match=r"noises\[2\]"):
        G.synthesis(wp, noises=[n if i != 2 else n.double() for i, n in enumerate(buffers(G))])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", ["shared", "rows"])
@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_noise_grad_vs_reference_golden(cd, form, mode):
    """d<image, gimg>/d noise of every conv layer at B = 2: shared maps (the reference as it is, its buffers as leaves) and a map
    per row (the reference run one row at a time).  The bound is grad_wp's, and like it (one figure over all of wp's rows) it is
    taken over the whole gradient, all maps together, as relative L2; the worst single map is printed beside it (bf16, measured:
    8.5e-2 on an 8 x 8 map of the per-row form, 64 elements a row, against 4.8e-2 over all maps; f32: 1.5e-6 against 8.9e-7)."""
    g = golden("s2_noise_grad.npz")
    G = generator(cd)
    wp, gimg = wp_gimg()
    leaves = [n.requires_grad_(True) for n in (buffers(G) if form == "shared" else row_maps())]
    img = G.synthesis(wp, noises=leaves)["image"]
    from tests.test_s2_gpu import relerr
    assert relerr(img, g[f"image_{form}"]) < (2e-4 if cd == "f32" else 1.8e-2)          # (the forward bound of test_s2_gpu)
    (img * gimg).sum().backward()
    bound = 1e-3 if cd == "f32" else 8e-2
    per = [l2rel(n.grad, g[f"g_{form}{i}"]) for i, n in enumerate(leaves)]
    got = torch.cat([n.grad.reshape(-1) for n in leaves])
    ref = torch.cat([torch.as_tensor(g[f"g_{form}{i}"]).reshape(-1) for i in range(NL)])
    e = l2rel(got, ref.numpy())
    meas(f"s2_noise_grad.{cd}.{form}.{mode}", l2=e, worst_map=max(per))
    assert e < bound, (e, per)
    assert all(tuple(n.grad.shape) == tuple(n.shape) for n in leaves)


@pytest.mark.parametrize("det", [True, False])
def test_wp_grad_and_launches_do_not_change(det):
    """wp.grad has the same bits with and without noise gradients (deterministic mode; the default mode's atomics differ from run
    to run by themselves); without `noises` the launches are those of a generator that never heard of them; with the module's
    switch off no noise pass is launched; a map that does not require grad gets none."""
    from dge_amd import ops
    was = ops.is_deterministic()
    ops.set_deterministic(det)
    try:
        G = generator("f32")
        wp0, gimg = wp_gimg()

        def run(noises, switch=True, grad_out=None):
            wp = wp0.clone().requires_grad_(True)
            G.synthesis.noise_grad_enabled = switch
            ops.KERNEL_LOG = log = []
            try:
                img = G.synthesis(wp, **({} if noises is None else {"noises": noises, "noise_grad_out": grad_out}))["image"]
                (img * gimg).sum().backward()
            finally:
                ops.KERNEL_LOG = None
                G.synthesis.noise_grad_enabled = True
            return wp.grad, [n for n, _ in log]
        base, log0 = run(None)
        assert not any("noise_grad" in n for n in log0)
        fixed, log1 = run(buffers(G))          # maps given, none requires grad: today's launches
        assert log1 == log0
        leaves = [n.requires_grad_(True) for n in buffers(G)]
        with_ng, log2 = run(leaves)
        assert [n for n in log2 if n != "dge_s2_noise_grad"] == log0 and log2.count("dge_s2_noise_grad") == NL
        if det:
            assert torch.equal(base, fixed) and torch.equal(base, with_ng)
        first = [n.grad.clone() for n in leaves]
        # only the maps that ask: layers 0 and 7
        some = [n.requires_grad_(i in (0, 7)) for i, n in enumerate(buffers(G))]
        _, log3 = run(some)
        assert log3.count("dge_s2_noise_grad") == 2 and some[1].grad is None and torch.equal(some[7].grad, first[7])
        # the switch, read in backward
        off = [n.requires_grad_(True) for n in buffers(G)]
        g_off, log4 = run(off, switch=False)
        assert log4 == log0 and all(n.grad is None for n in off)
        if det:
            assert torch.equal(g_off, base)
        # noise_grad_out: written there instead of reaching .grad
        outs = [torch.full_like(n, float("nan")) for n in leaves]
        into = [n.requires_grad_(True) for n in buffers(G)]
        run(into, grad_out=outs)
        assert all(n.grad is None for n in into) and all(torch.equal(o, f) for o, f in zip(outs, first))
    finally:
        ops.set_deterministic(was)
