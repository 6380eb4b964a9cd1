"""StyleGAN2Generator.synthesis(styles=...): the StyleSpace codes as the input of the synthesis network and as a differentiable one.
The model is the 64^2 generator of tests/s2_noise_models.py; the styles' gradient is compared with the reference's autograd
(tests/golden/s2_styles.npz, tools/gen_golden_s2_styles.py: a forward hook on every `style` module makes the styles leaves)
inside the grad_wp bounds test_s2_noise_grad_gpu.py uses, as relative L2."""
import numpy as np
import pytest
import torch

from tests.conftest import MODES, golden, meas, with_fixture_params
from tests.s2_noise_models import S2N_KW, S2N_RES, s2n_state_dict
from tests.s2_style_models import S64_CHANNELS, S64_NAMES, S64_ROWS, split_blocks, styles_wp_gimg

pytestmark = pytest.mark.gpu
_G = {}


def l2rel(a, b):
    a = (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64).ravel()
    b = (b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)).astype(np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def generator(cd):
    """The fixture's generator (its conv biases moved off the leaky-relu kink for the fixture's forward), one per dtype."""
    if cd not in _G:
        import dge_amd
        G = dge_amd.StyleGAN2Generator(64, compute_dtype=cd, **S2N_KW).cuda()
        G.load_state_dict(with_fixture_params(s2n_state_dict(), golden("s2_styles.npz")))
        G.eval()
        for p in G.parameters():
            p.requires_grad_(False)
        _G[cd] = G
    return _G[cd]


def buffers(G, B):
    return [getattr(G.synthesis, f"layer{i}").noise.detach().reshape(1, r, r).expand(B, r, r).contiguous() for i, r in enumerate(S2N_RES)]


def wp_of(B):
    from tests.golden import recipe as R
    return R.randn("s2s.wp3", (3, 10, 512), 5)[:B].cuda().contiguous()


@pytest.mark.parametrize("with_noises", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_styles_of_wp_give_the_image_of_wp_to_the_bit(cd, B, with_noises):
    from dge_amd.style_codes import StyleCodes
    G = generator(cd)
    wp = wp_of(B)
    kw = {"noises": buffers(G, B)} if with_noises else {}
    with torch.no_grad():
        ref = G.synthesis(wp, **kw)
        codes = StyleCodes(G.synthesis, B, wp.device).set_from_wp(wp)
        out = G.synthesis(styles=codes, **kw)
        assert torch.equal(out["image"], ref["image"])
        assert torch.equal(G.synthesis(styles=codes.detached(), **kw)["image"], ref["image"])          # the flat tensor itself
    assert "wp" not in out and set(out) == set(ref) - {"wp"}
    for k in out:
        assert torch.equal(out[k], ref[k]), k
    for name, blk in zip(codes.names, codes.blocks):          # the views are the blocks of the result dict
        key = f"style{int(name[5:]):02d}" if name.startswith("layer") else f"output_style{name[6:]}"
        assert torch.equal(blk, ref[key]), name
    # the saving forward (the flat leaf requires grad) gives the same image
    assert torch.equal(G.synthesis(styles=codes, **kw)["image"].detach(), ref["image"])


def test_styles_refuse_wp_and_malformed_buffers():
    from dge_amd.style_codes import StyleCodes
    G = generator("f32")
    wp = wp_of(1)
    codes = StyleCodes(G.synthesis, 1, wp.device).set_from_wp(wp)
    with pytest.raises(ValueError, match="takes the place of wp"):
        G.synthesis(wp, styles=codes)
    with pytest.raises(ValueError, match="flat tensor"):
        G.synthesis(styles=codes.detached()[:-1])
    with pytest.raises(ValueError, match="flat tensor"):
        G.synthesis(styles=codes.detached().double())
    with pytest.raises(ValueError, match="style_grad_out needs"):
        G.synthesis(wp, style_grad_out=codes.grads)
    with pytest.raises(ValueError, match="style_grad_out must be"):
        G.synthesis(styles=codes, style_grad_out=codes.grads[:-1])
    with pytest.raises(ValueError, match="give wp"):
        G.synthesis()
    with pytest.raises(ValueError, match="set_from_wp"):
        codes.set_from_wp(wp_of(3))


def _fixture_codes(G, g):
    from dge_amd.style_codes import StyleCodes
    wp = torch.as_tensor(g["wp"]).cuda()
    return wp, StyleCodes(G.synthesis, 2, wp.device).set_from_wp(wp)


@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_styles_and_image_vs_reference_golden(cd):
    """The styles dge_linear_rows forms and the image synthesised from them, inside the forward bounds of test_s2_noise_grad_gpu.py."""
    from tests.test_s2_gpu import relerr
    g = golden("s2_styles.npz")
    G = generator(cd)
    wp0, gimg0 = styles_wp_gimg()
    assert np.array_equal(g["wp"], wp0.numpy()) and np.array_equal(g["gimg"], gimg0.numpy())
    _, codes = _fixture_codes(G, g)
    with torch.no_grad():
        img = G.synthesis(styles=codes)["image"]
    m = dict(styles=relerr(codes.detached(), g["styles"]), image=relerr(img, g["image"]))
    meas(f"s2_styles.forward.{cd}", **m)
    bound = 2e-4 if cd == "f32" else 1.8e-2
    assert m["styles"] < 2e-4 and m["image"] < bound, m          # (the styles are f32 in both dtypes)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_style_grad_vs_reference_golden(cd, mode):
    """d<image, gimg> / d styles at B = 2 against the reference's autograd, as relative L2 over the whole gradient (the project's
    grad_wp bounds: 1e-3 f32, 8e-2 bf16), in both reduction modes; the worst single block is reported beside it.  Measured on the
    MI355X: see the README's parity table ("StyleSpace codes")."""
    g = golden("s2_styles.npz")
    G = generator(cd)
    _, codes = _fixture_codes(G, g)
    gimg = torch.as_tensor(g["gimg"]).cuda()
    img = G.synthesis(styles=codes)["image"]
    (img * gimg).sum().backward()
    got = codes.flat.grad
    assert got is not None and tuple(got.shape) == tuple(codes.flat.shape)
    e = l2rel(got, g["g_styles"])
    per = [l2rel(a, b) for a, b in zip(split_blocks(got.cpu().numpy(), 2), split_blocks(g["g_styles"], 2))]
    meas(f"s2_styles.grad.{cd}.{mode}", l2=e, worst_block=max(per), worst_block_name=S64_NAMES[int(np.argmax(per))])
    assert e < (1e-3 if cd == "f32" else 8e-2), (e, per)


@pytest.mark.parametrize("mode", MODES)
def test_wp_grad_is_the_affine_adjoint_of_the_style_grad_reference_chain_rule(mode):
    """s_g = W_g wp[:, row_g] * wscale + bias: wp.grad of the ordinary call equals sum over the blocks of a row of
    wscale * g_s_g @ W_g, formed in float64 on the host from the S form's gradient; within the f32 grad_wp bound (1e-3, relative L2)."""
    g = golden("s2_styles.npz")
    G = generator("f32")
    wp, codes = _fixture_codes(G, g)
    gimg = torch.as_tensor(g["gimg"]).cuda()
    (G.synthesis(styles=codes)["image"] * gimg).sum().backward()
    wpl = wp.clone().requires_grad_(True)
    (G.synthesis(wpl)["image"] * gimg).sum().backward()
    syn = G.synthesis
    mods = [getattr(syn, n) for n in S64_NAMES]
    ref = torch.zeros(2, 10, 512, dtype=torch.float64)
    for M, row, gs in zip(mods, S64_ROWS, split_blocks(codes.flat.grad.cpu().numpy(), 2)):
        ref[:, row] += M.style.wscale * (torch.as_tensor(gs).double() @ M.style.weight.detach().double().cpu())
    e = l2rel(wpl.grad, ref.numpy())
    meas(f"s2_styles.chain_rule.{mode}", l2=e)
    assert e < 1e-3, e


def test_style_grad_deterministic_bits_rows_and_grad_out():
    """Deterministic mode: the same bits on two runs; row b of a batch has the bits of the row run alone; style_grad_out receives
    the gradient INSTEAD of .grad; noise-map gradients beside it are those of the wp call."""
    from dge_amd import ops
    from dge_amd.style_codes import StyleCodes
    G = generator("f32")
    B = 3
    wp = wp_of(B)
    gimg = torch.as_tensor(golden("s2_styles.npz")["gimg"]).cuda()
    gimg = torch.cat([gimg, gimg[:1].flip(3)]).contiguous()
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        def run(wp_, gimg_, **kw):
            codes = StyleCodes(G.synthesis, wp_.shape[0], wp_.device).set_from_wp(wp_)
            (G.synthesis(styles=codes, **kw)["image"] * gimg_).sum().backward()
            return codes
        a, b = run(wp, gimg), run(wp, gimg)
        assert torch.equal(a.flat.grad, b.flat.grad) and float(a.flat.grad.abs().max()) > 0
        for row in range(B):
            one = run(wp[row:row + 1].contiguous(), gimg[row:row + 1].contiguous())
            for blk3, blk1, name in zip(split_blocks(a.flat.grad.cpu().numpy(), B), split_blocks(one.flat.grad.cpu().numpy(), 1), S64_NAMES):
                assert np.array_equal(blk3[row:row + 1], blk1), (row, name)
        c = StyleCodes(G.synthesis, B, wp.device).set_from_wp(wp)
        c.grads.fill_(float("nan"))
        (G.synthesis(styles=c, style_grad_out=c.grads)["image"] * gimg).sum().backward()
        assert c.flat.grad is None and torch.equal(c.grads, a.flat.grad)
        for blk, view in zip(split_blocks(c.grads.cpu().numpy(), B), c.grad_blocks):
            assert np.array_equal(blk, view.cpu().numpy())
        # noise maps beside the styles: their gradients are those of the wp call, the styles' gradient does not move
        n1 = [n.requires_grad_(True) for n in buffers(G, B)]
        d = run(wp, gimg, noises=n1)
        n2 = [n.requires_grad_(True) for n in buffers(G, B)]
        wpl = wp.clone().requires_grad_(True)
        (G.synthesis(wpl, noises=n2)["image"] * gimg).sum().backward()
        assert torch.equal(d.flat.grad, a.flat.grad)
        assert all(torch.equal(x.grad, y.grad) for x, y in zip(n1, n2))
    finally:
        ops.set_deterministic(was)


@pytest.mark.parametrize("det", [True, False])
def test_plain_wp_backward_is_untouched_by_a_styles_call(det):
    """A synthesis(wp) forward + backward before and after a `styles` call in the same process: the same KERNEL_LOG and the same
    conv-family launches (ops.PROFILE's shape tags: at 64^2 the default mode's chain logs nothing else), and (deterministic mode; the
    default mode's atomics differ from run to run by themselves) the same wp.grad bits.  The S form logs its own ending,
    dge_s2_style_grads_s, and no dge_linear_rows."""
    from dge_amd import ops
    G = generator("f32")
    g = golden("s2_styles.npz")
    gimg = torch.as_tensor(g["gimg"]).cuda()
    was = ops.is_deterministic()
    ops.set_deterministic(det)

    def logged(fn):
        ops.KERNEL_LOG, ops.PROFILE = log, prof = [], []
        try:
            out = fn()
        finally:
            ops.KERNEL_LOG = ops.PROFILE = None
        return out, ([n for n, _ in log], [e[3] for e in prof])

    def plain():
        wp = torch.as_tensor(g["wp"]).cuda().requires_grad_(True)
        (G.synthesis(wp)["image"] * gimg).sum().backward()
        return wp.grad
    try:
        plain()          # (the first call packs the weights)
        g0, log0 = logged(plain)
        _, codes = _fixture_codes(G, g)
        _, log_s = logged(lambda: (G.synthesis(styles=codes)["image"] * gimg).sum().backward())
        g1, log1 = logged(plain)
    finally:
        ops.set_deterministic(was)
    assert log0 == log1 and len(log0[1]) > 0
    assert log_s[0].count("s2_style_grads_s") == 1 and not any("linear_rows" in n for n in log_s[0])
    assert "s2_style_grads_s" not in log0[0] and log_s[1] == log0[1]          # (the S form runs the conv launches of the wp form)
    if det:
        assert torch.equal(g0, g1)


def test_style_sigma_and_an_edit_move_the_image():
    """infer.style_sigma on 96 samples against float64 statistics of the same styles, and a +3 sigma edit of one channel through the
    files' format: rows -> edit_styles -> load_rows -> synthesis."""
    from dge_amd.autograd_s2 import styles_from_wp
    from dge_amd.infer import edit_styles, style_sigma
    import dge_amd
    from dge_amd.style_codes import StyleCodes
    from tests.projector_models import PROJ_KW, proj_state_dict
    # (the projector tests' model: its mapping network is at a real checkpoint's scale - that of s2_noise_models gives every z
    # nearly the same w, and a std of 0 measures nothing)
    G = dge_amd.StyleGAN2Generator(64, compute_dtype="f32", **PROJ_KW).cuda()
    G.load_state_dict(proj_state_dict())
    G.eval()
    N = 96
    mean, sigma = style_sigma(G, samples=N, seed=3, chunk=40)
    assert [tuple(m.shape) for m in mean] == [(C,) for C in S64_CHANNELS] == [tuple(s.shape) for s in sigma]
    z = torch.randn(N, 512, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        w = G.mapping(z)["w"].float()
        flat = styles_from_wp(G.synthesis, w.unsqueeze(1).repeat(1, 10, 1).contiguous())
    for blk, m, s in zip(split_blocks(flat.cpu().numpy(), N), mean, sigma):
        b64 = blk.astype(np.float64)
        assert np.abs(m.cpu().numpy() - b64.mean(0)).max() < 1e-6 * np.abs(b64).max()
        assert b64.std(0).max() > 1e-3 and np.abs(s.cpu().numpy() - b64.std(0)).max() < 1e-5 * b64.std(0).max()
    wp = wp_of(1)
    codes = StyleCodes(G.synthesis, 1, wp.device).set_from_wp(wp)
    with torch.no_grad():
        before = G.synthesis(styles=codes)["image"].clone()
        rows = codes.rows(0)
        codes.load_rows(0, edit_styles(rows, "layer6", 5, 3.0, sigma))
        assert float(codes.blocks[6][0, 5] - rows[6][0, 5]) == pytest.approx(3.0 * float(sigma[6][5]), rel=1e-5)
        after = G.synthesis(styles=codes)["image"]
        assert not torch.equal(before, after)
        codes.load_rows(0, rows)
        assert torch.equal(G.synthesis(styles=codes)["image"], before)
