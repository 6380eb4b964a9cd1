"""The three kernels of the noise-map optimisation (csrc/s2_noise_kernels.hip) per operation, against float64 restatements on the
same operands: ops.s2_noise_grad (forms A and B, shared and per-row maps), ops.noise_reg (value and gradient over one table that
mixes map sizes) and ops.noise_normalize.  Inputs are rounded to the storage dtype first, so only the f32 accumulation is judged:
within 1e-6 of the largest reference element, the project's f32-against-float64 bound (tests/test_pn_act_bwd_gpu.py).  Equal bits
from call to call in both reduction modes, and for a row alone or inside a batch."""
import pytest
import torch

from tests.conftest import meas
from tests.golden import recipe as R
from tests.s2_noise_models import normalize_ref, reg_ref

pytestmark = pytest.mark.gpu

GAIN = 2.0 ** 0.5
# 4^2, 8^2, 64^2 and 3 pixels: fewer than one workgroup covers at every channel count but 512 in f32 (2 pixels per workgroup)
_SIZES = [(4, 4), (8, 8), (64, 64), (1, 3)]
_CHANNELS = [32, 64, 128, 512]
_SIDES = [4, 8, 16, 64]
# relative error of the scalar reg against float64: 4x the largest value measured on the MI355X (README, "Noise optimisation");
# the two means of a level cancel to about 1/sqrt(N) of their terms, so the scalar carries far fewer good digits than its terms
REG_REL_BOUND = 4 * 8.05e-8


def _operands(cd, B, H, W, Cc):
    """g and x in the compute dtype; about one entry of x in eight is exactly 0 (and stays 0 in bf16)."""
    dt = torch.float32 if cd == "f32" else torch.bfloat16
    x = R.randn(f"s2n.x.{B}.{H}.{W}.{Cc}", (B, H, W, Cc), 91)
    zero = R.randn(f"s2n.zero.{B}.{H}.{W}.{Cc}", (B, H, W, Cc), 92) > 1.15
    x = torch.where(zero, torch.zeros(()), x).to(dt)
    g = R.randn(f"s2n.g.{B}.{H}.{W}.{Cc}", (B, H, W, Cc), 93).to(dt)
    assert int((x == 0).sum()) > 0
    return g.cuda(), x.cuda()


def _ref64(g, x, ns, shared):
    """ns * sum_c g_z, g_z = g (form A) or g * gain * lrelu'(x), lrelu'(x) = 1 for x > 0 and 0.2 otherwise (at 0 too); a shared map
    sums the rows."""
    gz = g.double() if x is None else g.double() * GAIN * torch.where(x > 0, 1.0, 0.2).double()
    r = float(ns) * gz.sum(dim=-1).reshape(g.shape[0], -1)
    return r.sum(dim=0, keepdim=True) if shared else r


@pytest.mark.parametrize("form", ["A", "B"])
@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_noise_grad_against_float64(cd, form):
    from dge_amd import ops
    ns = torch.tensor([-0.37], device="cuda")
    worst = 0.0
    for B in (1, 3):
        for H, W in _SIZES:
            for Cc in _CHANNELS:
                g, x = _operands(cd, B, H, W, Cc)
                xa = x if form == "B" else None
                for shared in (True, False):
                    out = torch.full((1 if shared else B, H * W), float("nan"), device="cuda")          # (nothing pre-zeroed)
                    ops.KERNEL_LOG = log = []
                    try:
                        ops.s2_noise_grad(g, xa, GAIN, ns, out)
                    finally:
                        ops.KERNEL_LOG = None
                    assert [n for n, _ in log] == ["dge_s2_noise_grad"] and ops.last_kernel() == f"s2_noise_grad<{cd},{form}>"
                    ref = _ref64(g, xa, ns, shared)
                    err = ((out.double() - ref).abs().max() / ref.abs().max()).item()
                    worst = max(worst, err)
                    assert err <= 1e-6, (B, H, W, Cc, shared, err)
                    # accumulate: out += by the one writer of each element
                    acc = out.clone()
                    ops.s2_noise_grad(g, xa, GAIN, ns, acc, accumulate=True)
                    assert ((acc.double() - 2 * ref).abs().max() / ref.abs().max()).item() <= 2e-6
    meas("s2_noise_grad", cd=cd, form=form, err=worst)


def test_noise_grad_refuses_what_it_cannot_run():
    from dge_amd import ops
    ns = torch.tensor([0.1], device="cuda")
    with pytest.raises(ops.DgeError, match="unsupported channel count"):
        ops.s2_noise_grad(torch.zeros(1, 4, 4, 48, dtype=torch.bfloat16, device="cuda"), None, GAIN, ns)
    with pytest.raises(ops.DgeError, match="unsupported channel count"):
        ops.s2_noise_grad(torch.zeros(1, 4, 4, 2048, device="cuda"), None, GAIN, ns)
    with pytest.raises(ops.DgeError):
        ops.s2_noise_grad(torch.zeros(3, 4, 4, 32, device="cuda"), None, GAIN, ns, out=torch.zeros(2, 16, device="cuda"))


@pytest.mark.parametrize("det", [False, True])
def test_noise_grad_bits_repeat_and_rows_stand_alone(det):
    """Two calls give equal bits in either reduction mode (the kernel has no atomics and reads no mode), and row b of a per-row
    call equals the call on row b alone; the pixel that spans two waves (512 f32 channels) included."""
    from dge_amd import ops
    ns = torch.tensor([0.21], device="cuda")
    was = ops.is_deterministic()
    ops.set_deterministic(det)
    try:
        for cd, Cc, (H, W) in (("f32", 512, (8, 8)), ("bf16", 512, (8, 8)), ("bf16", 32, (64, 64)), ("f32", 64, (1, 3))):
            g, x = _operands(cd, 3, H, W, Cc)
            for xa in (None, x):
                for Bn in (1, 3):
                    a = ops.s2_noise_grad(g, xa, GAIN, ns, torch.empty(Bn, H * W, device="cuda"))
                    b = ops.s2_noise_grad(g, xa, GAIN, ns, torch.empty(Bn, H * W, device="cuda"))
                    assert torch.equal(a, b)
                for r in range(3):
                    one = ops.s2_noise_grad(g[r:r + 1].contiguous(), None if xa is None else xa[r:r + 1].contiguous(), GAIN, ns,
                                            torch.empty(1, H * W, device="cuda"))
                    assert torch.equal(one[0], a[r]), (cd, Cc, r)
    finally:
        ops.set_deterministic(was)


# ------------------------------------------------------------------ regulariser and renormalisation
def _table(sides, Bn, seed=9):
    """(table, flat leaf, the maps as [Bn, R, R] float64 host tensors): the maps are not centred and not of unit variance."""
    from dge_amd import ops
    tab = ops.NoiseTable(sides, Bn, "cuda")
    flat = torch.empty(tab.numel, device="cuda")
    maps = []
    for m, r in enumerate(sides):
        n = R.randn(f"s2n.map{m}.{r}", (3, r, r), seed, 1.3, 0.2)[:Bn]
        tab.view(flat, m).copy_(n)
        maps.append(n.double())
    return tab, flat, maps


@pytest.mark.parametrize("Bn", [1, 3])
def test_noise_reg_value_and_gradient_against_float64_autograd(Bn):
    """One table mixing R = 4, 8, 16, 64 (1, 1, 2 and 4 levels; the 64^2 map is the only one of more than one chunk): reg [Bn] and
    the gradient w.r.t. every map against torch float64 autograd of the restated formula."""
    from dge_amd import ops
    tab, flat, maps = _table(_SIDES, Bn)
    leaves = [n.clone().requires_grad_(True) for n in maps]
    ref = sum(reg_ref(n) for n in leaves)          # [Bn]
    ref.sum().backward()
    grad = torch.full_like(flat, float("nan"))
    reg = ops.noise_reg(tab, flat, grad=grad, scale=1.0)
    rel = ((reg.double().cpu() - ref.detach()).abs() / ref.detach().abs()).max().item()
    meas("noise_reg.value", Bn=Bn, rel=rel)
    assert rel <= REG_REL_BOUND, (rel, reg.tolist(), ref.tolist())
    gmax = max(float(n.grad.abs().max()) for n in leaves)
    for m, n in enumerate(leaves):
        err = ((tab.view(grad, m).double().cpu() - n.grad).abs().max() / gmax).item()
        meas("noise_reg.grad", Bn=Bn, R=_SIDES[m], err=err)
        assert err <= 1e-6, (m, err)          # of the largest gradient element of the table
    # scale and accumulate: grad (+)= scale * d reg
    g2 = grad.clone()
    ops.noise_reg(tab, flat, grad=g2, scale=3.0, accumulate=True)
    assert ((g2 - 4 * grad).abs().max() / grad.abs().max()).item() <= 1e-6
    # value alone
    assert torch.equal(ops.noise_reg(tab, flat), reg)


def test_noise_reg_levels_behind_the_second_pooling_pass():
    """A 512^2 map has seven levels: the sixth comes from the second pooling launch (from level 5, 16 x 16)."""
    from dge_amd import ops
    tab, flat, maps = _table([512, 8], 1, seed=10)
    assert ops.noise_levels(512) == 7 and tab.plan.n_pool1 == 1
    leaves = [n.clone().requires_grad_(True) for n in maps]
    ref = sum(reg_ref(n) for n in leaves)
    ref.sum().backward()
    grad = torch.full_like(flat, float("nan"))
    reg = ops.noise_reg(tab, flat, grad=grad)
    rel = (abs(float(reg[0]) - float(ref[0])) / abs(float(ref[0])))
    gmax = max(float(n.grad.abs().max()) for n in leaves)
    err = max(((tab.view(grad, m).double().cpu() - n.grad).abs().max() / gmax).item() for m, n in enumerate(leaves))
    meas("noise_reg.512", rel=rel, grad_err=err)
    assert rel <= REG_REL_BOUND and err <= 1e-6, (rel, err)


@pytest.mark.parametrize("Bn", [1, 3])
def test_noise_normalize_against_float64(Bn):
    from dge_amd import ops
    tab, flat, maps = _table(_SIDES, Bn)
    ops.noise_normalize(tab, flat)
    for m, n in enumerate(maps):
        got = tab.view(flat, m).double().cpu()
        ref = normalize_ref(n)
        err = ((got - ref).abs().max() / ref.abs().max()).item()
        mean, msq = got.mean(dim=(1, 2)).abs().max().item(), ((got * got).mean(dim=(1, 2)) - 1).abs().max().item()
        meas("noise_normalize", Bn=Bn, R=_SIDES[m], err=err, mean=mean, msq=msq)
        assert err <= 1e-6, (m, err)
        assert mean <= 1e-6 and msq <= 1e-6, (m, mean, msq)          # zero mean, unit mean square: to f32 rounding of values of size 1


@pytest.mark.parametrize("det", [False, True])
def test_reg_and_normalize_bits_repeat_and_rows_stand_alone(det):
    from dge_amd import ops
    was = ops.is_deterministic()
    ops.set_deterministic(det)
    try:
        tab, flat, maps = _table(_SIDES, 3)
        g1, g2 = torch.empty_like(flat), torch.empty_like(flat)
        r1, r2 = ops.noise_reg(tab, flat, grad=g1).clone(), ops.noise_reg(tab, flat, grad=g2).clone()
        assert torch.equal(r1, r2) and torch.equal(g1, g2)
        f1, f2 = flat.clone(), flat.clone()
        ops.noise_normalize(tab, f1)
        ops.noise_normalize(tab, f2)
        assert torch.equal(f1, f2)
        one = ops.NoiseTable(_SIDES, 1, "cuda")
        for b in range(3):
            fb = torch.empty(one.numel, device="cuda")
            for m in range(len(_SIDES)):
                one.view(fb, m).copy_(tab.view(flat, m)[b:b + 1])
            gb = torch.empty_like(fb)
            rb = ops.noise_reg(one, fb, grad=gb)
            assert torch.equal(rb[0], r1[b]), b
            ops.noise_normalize(one, fb)
            for m in range(len(_SIDES)):
                assert torch.equal(one.view(gb, m)[0], tab.view(g1, m)[b]), (b, m)
                assert torch.equal(one.view(fb, m)[0], tab.view(f1, m)[b]), (b, m)
    finally:
        ops.set_deterministic(was)


def test_noise_table_refuses_bad_maps_and_buffers():
    from dge_amd import ops
    with pytest.raises(ops.DgeError):
        ops.NoiseTable([12], 1, "cuda")
    with pytest.raises(ops.DgeError):
        ops.NoiseTable([2048], 1, "cuda")
    tab = ops.NoiseTable([4, 8], 1, "cuda")
    with pytest.raises(ops.DgeError):
        ops.noise_reg(tab, torch.zeros(tab.numel + 1, device="cuda"))
    with pytest.raises(ops.DgeError):
        ops.noise_normalize(tab, torch.zeros(tab.numel, device="cuda", dtype=torch.float64))
