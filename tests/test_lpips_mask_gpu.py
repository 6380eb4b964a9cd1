"""LPIPS.value_and_grad(mask=...) on the HIP kernels against the float64 restatement (tests/masked_lpips_ref.py) with the seeded
stand-in weights, at the shapes and inside the bounds of tests/test_lpips_gpu.py; exact independence of what lies under the mask;
the unmasked call untouched."""
import pytest
import torch

from oracle import lpips_ref as LR
from tests.conftest import meas
from tests.golden import recipe as R
from tests.masked_lpips_ref import masked_value_and_grad

pytestmark = pytest.mark.gpu

CASES = [("f32", (2, 3, 48, 40)), ("f32", (1, 3, 44, 44)), ("bf16", (1, 3, 64, 64))]
TOL = {"f32": (2e-4, 5e-3), "bf16": (3e-2, 0.25)}          # value, gradient L2: tests/test_lpips_gpu.py's, not widened


def model(cd):
    from dge_amd.lpips import LPIPS
    m = LPIPS(compute_dtype=cd).cuda()
    m.load_state_dict(LR.seeded_params(0))
    return m


def images(shape):
    a = R.randn("lp.a", shape, 4, 0.5).clamp(-1, 1)
    b = (a * 0.7 + R.randn("lp.b", shape, 4, 0.3)).clamp(-1, 1)
    return a, b


def make_mask(kind, shape):
    B, _, h, w = shape
    if kind == "soft":
        return torch.rand(B, 1, h, w, generator=torch.Generator().manual_seed(h * w + B))
    m = torch.ones(B, 1, h, w)          # the binary half-plane
    m[..., w // 2:] = 0
    return m


_REF = {}


def reference(cd, shape, kind):
    """(a, b, mask, dist [B] f64, d mean / d b f64): computed once per case and shared"""
    key = (shape, kind)
    if key not in _REF:
        a, b = images(shape)
        m = make_mask(kind, shape)
        dist, g = masked_value_and_grad(LR.seeded_params(0), a, b, m)
        _REF[key] = (a, b, m, dist, g / shape[0])
    return _REF[key]


@pytest.mark.parametrize("kind", ["soft", "half"])
@pytest.mark.parametrize("cd,shape", CASES)
def test_masked_lpips_value_and_gradient_vs_restatement(cd, shape, kind):
    a, b, m, ref_dist, ref_g = reference(cd, shape, kind)
    LP = model(cd)
    val, gb = LP.value_and_grad(a.cuda(), b.cuda(), mask=m.cuda())
    rows, _ = LP.value_and_grad(a.cuda(), b.cuda(), need_grad=False, per_sample=True, mask=m.cuda())
    ref = float(ref_dist.mean())
    ev = abs(float(val) - ref) / abs(ref)
    er = float((rows.cpu().double() / ref_dist - 1).abs().max())
    eg = float((gb.cpu().double() - ref_g).norm() / ref_g.norm())
    meas(f"lpips_mask.{cd}.{shape[2]}x{shape[3]}.{kind}", value=ev, rows=er, grad_l2=eg)
    tol_v, tol_g = TOL[cd]
    assert ev < tol_v, (float(val), ref)
    assert er < tol_v, (rows.tolist(), ref_dist.tolist())
    assert eg < tol_g, eg
    if kind == "half":
        assert not bool((gb[..., shape[3] // 2:] != 0).any())


@pytest.mark.parametrize("cd,shape", CASES)
def test_all_ones_mask_is_lpips(cd, shape):
    """m = 1 is LPIPS as it is: against the unmasked call, inside the bounds of the comparison with the restatement"""
    a, b = images(shape)
    LP = model(cd)
    v0, g0 = LP.value_and_grad(a.cuda(), b.cuda(), per_sample=True)
    v1, g1 = LP.value_and_grad(a.cuda(), b.cuda(), per_sample=True, mask=torch.ones(shape[0], 1, *shape[2:], device="cuda"))
    ev = float((v1 / v0 - 1).abs().max())
    eg = float((g1 - g0).norm() / g0.norm())
    meas(f"lpips_mask.ones.{cd}.{shape[2]}x{shape[3]}", value=ev, grad_l2=eg, grad_bits_equal=str(torch.equal(g0, g1)))
    assert ev < TOL[cd][0] and eg < TOL[cd][1], (ev, eg)


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("cd,shape", CASES)
def test_what_lies_under_the_mask_cannot_reach_the_result(cd, shape, det):
    """A binary mask; the target's pixels where m == 0 replaced by other values: the same bits of dist and gradient, and a gradient
    that is exactly 0 under the mask"""
    from dge_amd import ops
    a, b = images(shape)
    B, _, h, w = shape
    g = torch.Generator().manual_seed(17)
    m = (torch.rand(B, 1, h // 4, w // 4, generator=g) > 0.4).float().repeat_interleave(4, 2).repeat_interleave(4, 3)
    m[..., : w // 3] = 0
    hole = (m == 0).expand(-1, 3, -1, -1)
    a2 = torch.where(hole, torch.rand(shape, generator=g) * 2 - 1, a)
    assert not torch.equal(a, a2) and torch.equal(a * m, a2 * m)
    LP = model(cd)
    was = ops.is_deterministic()
    ops.set_deterministic(det)
    try:
        v1, g1 = LP.value_and_grad(a.cuda(), b.cuda(), per_sample=True, mask=m.cuda())
        v2, g2 = LP.value_and_grad(a2.cuda(), b.cuda(), per_sample=True, mask=m.cuda())
    finally:
        ops.set_deterministic(was)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    assert not bool((g1.cpu()[hole] != 0).any()) and bool((g1 != 0).any())
    assert bool((v1 > 0).all())


def test_empty_mask_row_gives_zero_and_state_refills_in_place():
    cd, shape = "f32", (2, 3, 48, 40)
    a, b = images(shape)
    LP = model(cd)
    m = make_mask("soft", shape)
    m[1] = 0
    st = LP.mask_state(m.cuda())
    v, g = LP.value_and_grad(a.cuda(), b.cuda(), per_sample=True, mask_state=st)
    assert float(v[1]) == 0.0 and not bool((g[1] != 0).any()) and float(v[0]) > 0 and bool(torch.isfinite(g).all())
    assert float(st.cover()[1]) == 0.0 and abs(float(st.cover()[0]) - float(m[0].mean())) < 1e-6
    # set(): the storage is refilled, the addresses stay, the result has the bits of a fresh state
    m2 = make_mask("half", shape)
    ptrs = [x.data_ptr() for x in st.levels] + [st.inv_sum.data_ptr(), st.slots.data_ptr()]
    st.set(m2.cuda())
    assert ptrs == [x.data_ptr() for x in st.levels] + [st.inv_sum.data_ptr(), st.slots.data_ptr()]
    v2, g2 = LP.value_and_grad(a.cuda(), b.cuda(), per_sample=True, mask_state=st)
    v3, g3 = LP.value_and_grad(a.cuda(), b.cuda(), per_sample=True, mask=m2.cuda())
    assert torch.equal(v2, v3) and torch.equal(g2, g3)
    with pytest.raises(ValueError, match="single-channel"):
        LP.value_and_grad(a[:, :1].cuda(), b[:, :1].cuda(), need_grad=False, mask=m[:, :, :, :].cuda())
    with pytest.raises(ValueError, match="mask state was made for"):
        LP.value_and_grad(a[:1].cuda(), b[:1].cuda(), mask_state=st)


def test_no_mask_issues_the_unmasked_launches_and_bits():
    """mask=None against a call that does not pass the keyword: the same KERNEL_LOG and the same bits; the masked call shows its
    launches in the log"""
    from dge_amd import ops
    cd, shape = "f32", (2, 3, 48, 40)
    a, b = images(shape)
    LP = model(cd)
    was = ops.is_deterministic()
    ops.set_deterministic(True)

    def logged(**kw):
        ops.KERNEL_LOG = log = []
        try:
            v, g = LP.value_and_grad(a.cuda(), b.cuda(), **kw)
        finally:
            ops.KERNEL_LOG = None
        return v.clone(), g.clone(), [n for n, _ in log]
    try:
        logged()          # (the first call packs the weights)
        v0, g0, log0 = logged()
        v1, g1, log1 = logged(mask=None, mask_state=None)
        _, _, logm = logged(mask=make_mask("soft", shape).cuda())
    finally:
        ops.set_deterministic(was)
    assert log0 == log1 and torch.equal(v0, v1) and torch.equal(g0, g1)
    new = ["dge_mask_pyramid", "dge_lpips_prep_masked", "dge_lpips_head_w", "dge_lpips_head_w_finalize", "dge_lpips_prep_bwd_masked"]
    assert not any(n in new for n in log0)
    assert [logm.count(n) for n in new] == [1, 2, 5, 1, 1]          # (the pyramid: mask= builds the state in the call)
    assert [n for n in logm if n not in new] == log0          # the VGG launches between them are the unmasked call's
