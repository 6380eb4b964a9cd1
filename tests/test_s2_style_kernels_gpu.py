"""dge_s2_style_grads_s and dge_cols_mean_std (csrc/s2_style_kernels.hip) against float64 restatements on the same random operands."""
import numpy as np
import pytest
import torch

from tests.conftest import meas

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # the unit roundoff of f32
# (kind, in_c, out_c, nslot_p, nslot_s): both tail loops of the o loop (out_c 5: one group of four and one left over; in_c 6 < one
# wave), a block wider than a wave, the widest the kernel takes, a toRGB block, and a finished block (st alone)
TABLE = (("conv", 8, 8, 1, 1), ("conv", 6, 5, 3, 3), ("conv", 64, 32, 3, 1), ("conv", 512, 512, 1, 3), ("rgb", 32, 0, 0, 0),
         ("done", 16, 0, 0, 3))
BSCALE = 0.7
# dge_cols_mean_std: the std against float64, relative to the largest std of the matrix.  Measured on the MI355X: 1.26e-7 (worst of
# the six shapes; README, "StyleSpace codes"); the bound is 4x that, as dge_rows_mean_std's row of the README sets its own.
COLS_STD_MEASURED = 1.26e-7
COLS_STD_BOUND = 4 * COLS_STD_MEASURED


def rnd(name, shape, scale=1.0):
    from tests.golden import recipe as R
    return R.randn("s2sk." + name, tuple(shape), 31, scale).cuda().contiguous()


def operands(B):
    """The table's operands for batch B; row b of every [.., B, ..] operand does not depend on B (seeded per block at B = 3, sliced)."""
    blocks = []
    for g, (kind, ic, oc, nsp, nss) in enumerate(TABLE):
        o = dict(kind=kind, in_c=ic, out_c=oc)
        if kind == "rgb":
            o["gs"] = rnd(f"{g}.gs", (3, ic))[:B].contiguous()
        else:
            o["st"] = rnd(f"{g}.st", (nss, 3, ic, 2))[:, :B].contiguous()
        if kind == "conv":
            o["P"] = rnd(f"{g}.P", (nsp, 3, oc, 2))[:, :B].contiguous()
            o["d"] = (rnd(f"{g}.d", (3, oc)).abs() + 0.5)[:B].contiguous()
            o["s"] = rnd(f"{g}.s", (3, ic))[:B].contiguous()
            o["bias"] = rnd(f"{g}.bias", (oc,), 0.3)
            o["wsq"] = rnd(f"{g}.wsq", (oc, ic)).square().contiguous()
        blocks.append(o)
    return blocks


def slot_stats(buf):
    from dge_amd import ops
    nslot, B, C, _ = buf.shape
    st = ops.SlotStats(B, C, buf.device)
    st.alloc(nslot).copy_(buf)
    return st


def launch(blocks, B, out=None):
    """dge_s2_style_grads_s over the table -> the flat buffer in the blocks' order (filled with NaN first: nothing is pre-zeroed)."""
    from dge_amd import ops
    total = sum(o["in_c"] for o in blocks)
    out = torch.full((B * total,), float("nan"), device="cuda") if out is None else out
    entries, off = [], 0
    for o in blocks:
        e = dict(out=out[B * off:B * (off + o["in_c"])].view(B, o["in_c"]))
        off += o["in_c"]
        if o["kind"] == "rgb":
            e["gs"] = o["gs"]
        else:
            e["st"] = slot_stats(o["st"])
        if o["kind"] == "conv":
            e.update(P=slot_stats(o["P"]), d=o["d"], s=o["s"], bias=o["bias"], wsq=o["wsq"], bscale=BSCALE)
        entries.append(e)
    ops.s2_style_grads_s(entries, B)
    return out


def reference(o):
    """float64: (g_s [B,in_c], the magnitude sum of the bound [B,in_c])"""
    f = lambda t: t.double().cpu()
    if o["kind"] == "rgb":
        return f(o["gs"]), f(o["gs"]).abs()
    st0 = f(o["st"])[..., 0]
    if o["kind"] == "done":
        return st0.sum(0), st0.abs().sum(0)
    P = f(o["P"]).sum(0)
    t = -(P[..., 0] - f(o["bias"]) * BSCALE * P[..., 1]) * f(o["d"]) ** 2          # [B,out_c]
    wsq, s = f(o["wsq"]), f(o["s"])
    return st0.sum(0) + s * (t @ wsq), st0.abs().sum(0) + s.abs() * (t.abs() @ wsq)


@pytest.mark.parametrize("B", [1, 3])
def test_style_grads_s_against_float64(B):
    """Every block of the table in ONE launch, against float64 on the same operands.  The bound is derived, per element:

        (out_c + nslot_p + nslot_s + 8) * 2^-24 * (sum_slots |st| + |s| * sum_o |t_o * wsq_oc|)

    Every f32 operation rounds by at most 2^-24 of its result, and the results along the way are bounded by the magnitude sum in the
    bracket.  Counting roundings on the path to one element: the slot copies of P and of st are added in turn (nslot_p - 1 and
    nslot_s - 1 additions); t_o takes four (bias * bscale, the fused multiply-subtract, and the two multiplications by d); the
    sum over o is out_c fused multiply-adds spread over four accumulators (at most out_c / 4 + 1 roundings on the longest chain, and
    three more to join the accumulators: fewer than out_c + 2 in all); the product with s and the addition of st take two.  That
    is fewer than out_c + nslot_p + nslot_s + 8.  A toRGB block and a finished block with one slot are copies: the bound is met
    with equality at 0."""
    blocks = operands(B)
    got = launch(blocks, B).cpu().double()
    assert not torch.isnan(got).any()          # every (block, b, c) was written
    off, worst = 0, 0.0
    for o, (kind, ic, oc, nsp, nss) in zip(blocks, TABLE):
        ref, mag = reference(o)
        g = got[B * off:B * (off + ic)].view(B, ic)
        off += ic
        bound = (oc + nsp + nss + 8) * U * mag
        err = (g - ref).abs()
        if kind == "rgb":
            assert torch.equal(g, ref)
        ratio = float((err / bound.clamp_min(1e-300)).max())
        meas(f"s2_style_grads_s.B{B}.{kind}.{ic}x{oc}", err_over_bound=ratio, err=float(err.max()), rel=float((err / mag.clamp_min(1e-300)).max()))
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), (kind, ic, oc, ratio)
    meas(f"s2_style_grads_s.B{B}.worst", err_over_bound=worst)


def test_style_grads_s_ties_to_the_wp_ending():
    """g_wp of dge_s2_style_grads on the same table (the conv and toRGB blocks; two blocks share a row, as layer 2k+1 and toRGB k
    do) against wscale * g_s @ Wstyle formed in float64 from the NEW kernel's g_s.  The two kernels share the device code of g_s
    (s2_style_steps.h), so what is left is the contraction: in_c fused multiply-adds in four accumulators, three additions to
    join them, the product with wscale and the atomic addition onto g_wp (one more per block of the row) - per element fewer than
    (in_c + 8) * 2^-24 * wscale * sum_c |g_s[c] * W[c,k]|, summed over the blocks of the row."""
    from dge_amd import ops
    B, K, nrows, wscale = 3, 512, 6, 0.37
    blocks = [o for o in operands(B) if o["kind"] != "done"]
    rows = [0, 2, 3, 5, 3]          # the toRGB block shares row 3 with the (64,32) conv block
    gs = launch(blocks, B).cpu().double()
    entries = []
    for g, (o, row) in enumerate(zip(blocks, rows)):
        o["wstyle"] = rnd(f"{g}.wstyle", (o["in_c"], K), 0.2)
        e = dict(wstyle=o["wstyle"], row=row)
        if o["kind"] == "rgb":
            e["gs"] = o["gs"]
        else:
            e.update(P=slot_stats(o["P"]), st=slot_stats(o["st"]), d=o["d"], s=o["s"], bias=o["bias"], wsq=o["wsq"], bscale=BSCALE)
        entries.append(e)
    g_wp = ops.s2_style_grads(entries, torch.zeros((B, nrows, K), device="cuda"), wscale).cpu().double()
    ref, bound, off = torch.zeros(B, nrows, K, dtype=torch.float64), torch.zeros(B, nrows, K, dtype=torch.float64), 0
    for o, row in zip(blocks, rows):
        ic = o["in_c"]
        g = gs[B * off:B * (off + ic)].view(B, ic)
        off += ic
        W = o["wstyle"].double().cpu()
        ref[:, row] += wscale * (g @ W)
        bound[:, row] += (ic + 8) * U * wscale * (g.abs() @ W.abs())
    err = (g_wp - ref).abs()
    assert float(g_wp[:, 1].abs().max()) == 0.0 and float(g_wp[:, 4].abs().max()) == 0.0          # rows no block names stay zero
    ratio = float((err / bound.clamp_min(1e-300))[:, rows].max())
    meas("s2_style_grads.vs_s_form", err_over_bound=ratio, err=float(err.max()))
    assert bool((err <= bound).all()), ratio


def test_style_grads_s_same_bits_on_a_second_call_and_for_a_row_alone():
    blocks = operands(3)
    a, b = launch(blocks, 3), launch(blocks, 3)
    assert torch.equal(a, b)
    total = sum(o["in_c"] for o in blocks)
    for row in range(3):
        one = []
        for o in blocks:
            p = dict(o)
            for k in ("st", "P"):
                if k in p:
                    p[k] = p[k][:, row:row + 1].contiguous()
            for k in ("gs", "d", "s"):
                if k in p:
                    p[k] = p[k][row:row + 1].contiguous()
            one.append(p)
        alone = launch(one, 1)
        off = 0
        for o in blocks:
            ic = o["in_c"]
            assert torch.equal(alone[off:off + ic], a[3 * off:3 * (off + ic)].view(3, ic)[row]), (row, o["kind"], ic)
            off += ic
        assert off == total


def test_style_grads_s_refuses_bad_tables():
    from dge_amd import ops
    from dge_amd._lib import DgeError
    out = torch.zeros(2 * 8, device="cuda").view(2, 8)
    with pytest.raises(DgeError, match="1..32 blocks"):
        ops.s2_style_grads_s([], 2)
    with pytest.raises(DgeError, match="one shape"):
        ops.s2_style_grads_s([dict(gs=torch.zeros((2, 4), device="cuda"), out=out)], 2)
    with pytest.raises(DgeError, match="bad block 0"):
        ops.s2_style_grads_s([dict(gs=torch.zeros((2, 513), device="cuda"), out=torch.zeros((2, 513), device="cuda"))], 2)


@pytest.mark.parametrize("N", [1, 7, 1025])
@pytest.mark.parametrize("D", [8, 515])
def test_cols_mean_std_against_float64(N, D):
    """Mean: within 1e-6 of the matrix's largest element (the project's bound for dge_rows_mean_std).  Std: relative to the largest
    std, inside COLS_STD_BOUND.  One row: the std is exactly 0.  The same bits on a second call."""
    from dge_amd import ops
    x = (rnd(f"cols.{N}.{D}", (N, D), 1.3) + 0.4 * torch.arange(D, device="cuda").remainder(7)).contiguous()
    mean, std = ops.cols_mean_std(x)
    mean2, std2 = ops.cols_mean_std(x)
    assert torch.equal(mean, mean2) and torch.equal(std, std2)
    x64 = x.double().cpu()
    rm = x64.mean(0)
    rs = ((x64 - rm) ** 2).sum(0).div(N).sqrt()
    em = float((mean.cpu().double() - rm).abs().max() / x64.abs().max())
    es = float((std.cpu().double() - rs).abs().max() / rs.max().clamp_min(1e-300)) if N > 1 else float(std.abs().max())
    meas(f"cols_mean_std.{N}x{D}", mean=em, std=es)
    assert em < 1e-6, em
    if N == 1:
        assert es == 0.0
    else:
        assert es < COLS_STD_BOUND, es
