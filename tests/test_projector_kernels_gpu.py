"""The kernels of csrc/projector_kernels.hip one by one, at the smallest shapes where each can go wrong: dge_adam_multi against a
float64 restatement of its formula and against torch.optim.Adam on the CPU, dge_w_broadcast / dge_w_broadcast_bwd to the bit
against CPU torch, dge_rows_mean_std against float64, dge_area_pool_bwd against its closed form and as the transpose of the forward.
Every kernel gives the same bits in the default and the deterministic reduction mode and from run to run."""
import math

import pytest
import torch

from tests.conftest import meas
from tests.golden import recipe as R

pytestmark = pytest.mark.gpu

# largest relative error of p - p0 after three steps against the float64 restatement: 4x the value measured on the MI355X, 1.65e-6
# (README, "StyleGAN2 projector"; 1.83e-6 against torch.optim.Adam's own f32).  p itself is stored in f32: one rounding of a p of
# 2 .. 4 is 1.2e-7, 1e-6 of a total step of 0.1
ADAM_BOUND = 4 * 1.65e-6
# relative error of std against float64: 4x the largest value measured on the MI355X over the shapes below, 6.76e-8 (README)
STD_BOUND = 4 * 6.76e-8


def both_modes(fn):
    """fn() in the default and in the deterministic reduction mode (twice): the same bits -> the result"""
    from dge_amd import ops
    was = ops.is_deterministic()
    outs = []
    try:
        for on in (False, True, True):
            ops.set_deterministic(on)
            r = fn()
            outs.append([t.clone() for t in (r if isinstance(r, (list, tuple)) else [r])])
    finally:
        ops.set_deterministic(was)
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o))
    return outs[0]


# ------------------------------------------------------------------ dge_adam_multi
SIZES = (1, 3, 255, 256, 257, 1029)
LRS = (0.1, 0.0, 0.03)
B1, B2, EPS = 0.9, 0.999, 1e-8


def adam_inputs():
    p0 = [R.randn(f"proj.adam.p{i}", (n,), 21) for i, n in enumerate(SIZES)]
    gs = [[R.randn(f"proj.adam.g{k}.{i}", (n,), 22, 0.3) for i, n in enumerate(SIZES)] for k in range(len(LRS))]
    return p0, gs


def adam_device(p0, gs, scalars_on_device=False, offset=0):
    """Three dge_adam_multi steps; offset: the tensors are views `offset` floats into their buffers (1: no 16-byte alignment)."""
    from dge_amd import ops

    def dev(t):
        buf = torch.zeros(t.numel() + offset, dtype=torch.float32, device="cuda")
        v = buf[offset:]
        v.copy_(t)
        return v
    p, m, v = [dev(t) for t in p0], [dev(torch.zeros_like(t)) for t in p0], [dev(torch.zeros_like(t)) for t in p0]
    trace = []
    for k, lr in enumerate(LRS):
        t = k + 1
        step, isb = lr / (1 - B1 ** t), 1 / math.sqrt(1 - B2 ** t)
        g = [dev(x) for x in gs[k]]
        if scalars_on_device:
            ops.adam_multi(p, g, m, v, B1, B2, EPS, scalars=torch.tensor([step, isb], dtype=torch.float32).cuda())
        else:
            ops.adam_multi(p, g, m, v, B1, B2, EPS, step, isb)
        trace.append([x.clone() for x in p])
    return trace, m, v


def adam_f64(p0, gs):
    p, m, v = [x.double().clone() for x in p0], [torch.zeros_like(x).double() for x in p0], [torch.zeros_like(x).double() for x in p0]
    for k, lr in enumerate(LRS):
        t = k + 1
        for i in range(len(p)):
            g = gs[k][i].double()
            m[i] = B1 * m[i] + (1 - B1) * g
            v[i] = B2 * v[i] + (1 - B2) * g * g
            p[i] = p[i] - (lr / (1 - B1 ** t)) * m[i] / (v[i].sqrt() / math.sqrt(1 - B2 ** t) + EPS)
    return p, m, v


def test_adam_multi_against_float64_and_torch_adam():
    from dge_amd import ops
    p0, gs = adam_inputs()
    ops.KERNEL_LOG = log = []
    try:
        trace, m, v = adam_device(p0, gs)
    finally:
        ops.KERNEL_LOG = None
    assert [n for n, _ in log] == ["adam_multi"] * len(LRS)          # one launch per step for all six tensors
    ref_p, ref_m, ref_v = adam_f64(p0, gs)
    # torch.optim.Adam on the CPU in f32, the learning rate set per step
    tp = [x.clone().requires_grad_(True) for x in p0]
    opt = torch.optim.Adam(tp, lr=LRS[0], betas=(B1, B2), eps=EPS)
    for k, lr in enumerate(LRS):
        for grp in opt.param_groups:
            grp["lr"] = lr
        for x, g in zip(tp, gs[k]):
            x.grad = g.clone()
        opt.step()
    worst = dict(f64=0.0, torch=0.0, m=0.0, v=0.0)
    for i, n in enumerate(SIZES):
        d_ref = ref_p[i] - p0[i].double()
        got = trace[-1][i].cpu().double() - p0[i].double()
        worst["f64"] = max(worst["f64"], float((got - d_ref).abs().max() / d_ref.abs().max()))
        d_t = tp[i].detach().double() - p0[i].double()
        worst["torch"] = max(worst["torch"], float((got - d_t).abs().max() / d_t.abs().max()))
        worst["m"] = max(worst["m"], float((m[i].cpu().double() - ref_m[i]).abs().max() / ref_m[i].abs().max()))
        worst["v"] = max(worst["v"], float((v[i].cpu().double() - ref_v[i]).abs().max() / ref_v[i].abs().max()))
        assert trace[-1][i].numel() == n
    meas("projector.adam_multi", **worst)
    assert worst["f64"] < ADAM_BOUND and worst["torch"] < ADAM_BOUND, worst
    assert worst["m"] < 1e-6 and worst["v"] < 1e-6, worst          # three f32 updates of a moment: a few roundings of 6e-8
    # lr_t = 0 (the second step) leaves the bits of p, and moves the moments
    for a, b in zip(trace[0], trace[1]):
        assert torch.equal(a, b)
    assert not torch.equal(trace[1][-1], trace[2][-1])


def test_adam_multi_scalar_forms_alignment_and_modes():
    p0, gs = adam_inputs()
    host = both_modes(lambda: adam_device(p0, gs)[0][-1])
    plain = adam_device(p0, gs)
    dev = adam_device(p0, gs, scalars_on_device=True)
    odd = adam_device(p0, gs, offset=1)          # no tensor 16-byte aligned: the scalar loop alone
    for k in range(len(LRS)):
        for i in range(len(SIZES)):
            assert torch.equal(plain[0][k][i], dev[0][k][i]), (k, i)
            assert torch.equal(dev[0][k][i], odd[0][k][i]), (k, i)
    for i in range(len(SIZES)):
        assert torch.equal(host[i], dev[0][-1][i])
        assert torch.equal(dev[1][i], odd[1][i]) and torch.equal(dev[2][i], odd[2][i])


def test_adam_class_steps_like_torch_adam():
    """custom_adam.Adam over two tensors with a per-call learning rate against torch.optim.Adam on the CPU; graph_reset clears the
    state in place."""
    from dge_amd.custom_adam import Adam
    p0, gs = adam_inputs()
    idx = (3, 5)
    dp = [p0[i].cuda().requires_grad_(True) for i in idx]
    tp = [p0[i].clone().requires_grad_(True) for i in idx]
    opt, ref = Adam(dp, lr=0.5), torch.optim.Adam(tp, lr=0.5, betas=(B1, B2), eps=EPS)
    for k, lr in enumerate(LRS):
        for grp in ref.param_groups:
            grp["lr"] = lr
        for x, y, i in zip(dp, tp, idx):
            x.grad, y.grad = gs[k][i].cuda(), gs[k][i].clone()
        opt.step(lr=lr)
        ref.step()
    for x, y, i in zip(dp, tp, idx):
        d = y.detach().double() - p0[i].double()
        assert float((x.detach().cpu().double() - p0[i].double() - d).abs().max() / d.abs().max()) < ADAM_BOUND
    assert opt.t == 3 and all(st["step"] == 3 for st in opt.state.values())
    ptrs = [opt.state[x]["exp_avg"].data_ptr() for x in dp]
    opt.graph_reset()
    assert opt.t == 0 and ptrs == [opt.state[x]["exp_avg"].data_ptr() for x in dp]
    assert all(float(st["exp_avg"].abs().max()) == 0.0 and float(st["exp_avg_sq"].abs().max()) == 0.0 for st in opt.state.values())
    with pytest.raises(ValueError):
        Adam(dp, betas=(1.0, 0.999))


# ------------------------------------------------------------------ dge_w_broadcast / dge_w_broadcast_bwd
WB_SHAPES = [(B, L, D) for B in (1, 3) for L in (1, 10, 18) for D in (8, 512)]


@pytest.mark.parametrize("B,L,D", WB_SHAPES)
def test_w_broadcast_bits(B, L, D):
    from dge_amd import ops
    w, n = R.randn("proj.wb.w", (B, D), 31), R.randn("proj.wb.n", (B, D), 32)
    s = torch.tensor(0.69261199, dtype=torch.float32)
    wd, nd = w.cuda(), n.cuda()
    got = both_modes(lambda: ops.w_broadcast(wd, L, nd, float(s)))[0]
    want = (w + n * s).unsqueeze(1).expand(B, L, D)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(ops.w_broadcast(wd, L, nd, s.cuda().reshape(1)), got)          # the device-scalar form
    assert torch.equal(ops.w_broadcast(wd, L).cpu(), w.unsqueeze(1).expand(B, L, D))   # without noise
    assert ops.last_kernel() == "w_broadcast"


@pytest.mark.parametrize("B,L,D", WB_SHAPES)
def test_w_broadcast_bwd_bits_and_rows(B, L, D):
    from dge_amd import ops
    g = R.randn("proj.wb.g", (B, L, D), 33)
    gd = g.cuda()
    got = both_modes(lambda: ops.w_broadcast_bwd(gd))[0]
    seq = torch.zeros(B, D)
    for l in range(L):
        seq = seq + g[:, l]
    assert torch.equal(got.cpu(), seq)
    ref = g.double().sum(dim=1)
    assert float((got.cpu().double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    for b in range(B):
        assert torch.equal(ops.w_broadcast_bwd(gd[b:b + 1].contiguous()), got[b:b + 1])
    assert ops.last_kernel() == "w_broadcast_bwd"


def test_w_broadcast_is_differentiable_through_the_step_function():
    from dge_amd.projector import _WBroadcast
    w = R.randn("proj.wb.w", (3, 512), 31).cuda().requires_grad_(True)
    n = R.randn("proj.wb.n", (3, 512), 32).cuda()
    ws = _WBroadcast.apply(w, n, 0.25, 10)
    g = R.randn("proj.wb.g", (3, 10, 512), 33).cuda()
    ws.backward(g)
    seq = torch.zeros(3, 512)
    for l in range(10):
        seq = seq + g[:, l].cpu()
    assert torch.equal(w.grad.cpu(), seq)


# ------------------------------------------------------------------ dge_rows_mean_std
@pytest.mark.parametrize("N", (1, 7, 1025, 10000))
@pytest.mark.parametrize("D", (8, 512))
def test_rows_mean_std(N, D):
    from dge_amd import ops
    x = R.randn(f"proj.ms.{N}.{D}", (N, D), 41, 0.6, 0.3)
    xd = x.cuda()
    mean, std = both_modes(lambda: ops.rows_mean_std(xd))
    m64 = x.double().mean(dim=0)
    s64 = float((((x.double() - m64) ** 2).sum() / N).sqrt())
    err_m = float((mean.cpu().double() - m64).abs().max()) / float(x.abs().max())
    err_s = abs(float(std) - s64) / s64 if s64 > 0 else abs(float(std))
    meas(f"projector.rows_mean_std.{N}x{D}", mean=err_m, std=err_s)
    assert tuple(mean.shape) == (D,) and tuple(std.shape) == (1,)
    assert err_m <= 1e-6, err_m
    assert err_s <= STD_BOUND, err_s
    if N == 1:
        assert torch.equal(mean.cpu(), x[0]) and float(std) == 0.0
    assert ops.last_kernel() == "rows_mean_std"


def test_rows_mean_std_refuses_bad_sizes():
    from dge_amd import ops
    from dge_amd._lib import DgeError
    with pytest.raises(DgeError):
        ops.rows_mean_std(torch.zeros(4, 6, device="cuda"))          # D is no multiple of 4


# ------------------------------------------------------------------ dge_area_pool_bwd
@pytest.mark.parametrize("k", (1, 2, 4))
@pytest.mark.parametrize("S", (8, 16))
def test_area_pool_bwd(k, S):
    from dge_amd import ops
    B, C = 2, 3
    gp = R.randn(f"proj.pool.g{k}.{S}", (B, C, S // k, S // k), 51)
    x = R.randn(f"proj.pool.x{k}.{S}", (B, C, S, S), 52)
    gpd, xd = gp.cuda(), x.cuda()
    got = both_modes(lambda: ops.area_pool_bwd(gpd, k))[0]
    want = (gp / float(k * k)).repeat_interleave(k, dim=2).repeat_interleave(k, dim=3)
    assert torch.equal(got.cpu(), want)
    pooled = ops.area_pool(xd, k)
    lhs = float((pooled.cpu().double() * gp.double()).sum())
    rhs = float((x.double() * got.cpu().double()).sum())
    scale = float((x.double() * got.cpu().double()).abs().sum())          # (the inner product itself may cancel to near 0)
    assert abs(lhs - rhs) <= 1e-6 * scale, (lhs, rhs, scale)
    assert ops.last_kernel() == "area_pool_bwd"
