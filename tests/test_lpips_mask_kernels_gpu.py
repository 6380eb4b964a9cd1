"""The masked-LPIPS kernels (csrc/lpips_mask_kernels.hip), each against float64 on the same operands: the mask pyramid, the
weighted head with its finaliser, the masked input preparation and its adjoint, and the mask blend."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.conftest import meas

pytestmark = pytest.mark.gpu

ELEM_BOUND = 1e-6          # the project's bound for f32 element-wise kernels, of the largest element
# inv_sum [B,5] against 1 / (the float64 sum of the float64 levels), relative.  Measured on the MI355X over every case below:
# 1.45e-7 (worst: 48 x 40; 1.02e-7 .. 1.45e-7 over the five shapes - an f32 sum in tiles of 1024 and one rounded division, on
# levels that are themselves within 1.3e-7 of float64).  The bound is 4x that, the project's margin for scalar sums.
INV_SUM_MEASURED = 1.45e-7
INV_SUM_BOUND = 4 * INV_SUM_MEASURED
# dist of dge_lpips_head_w + dge_lpips_head_w_finalize against float64 on the same (rounded) operands, relative.  Measured on the
# MI355X over every case below: 2.41e-7 in f32 (C = 512) and 1.99e-7 in bf16 (C = 64): the features are rounded before both sides
# read them, so the dtype does not show.  4x the larger.
HEAD_DIST_MEASURED = 2.41e-7
HEAD_DIST_BOUND = 4 * HEAD_DIST_MEASURED
# Also measured there (asserted against ELEM_BOUND / one bf16 rounding below): levels 1.32e-7, g1 2.41e-7 of the largest in f32 and
# 3.3e-3 in bf16; with m = 1, g1 against dge_lpips_head's: 1.82e-7 of the largest in f32, where the bits are not equal (last-bit
# differences between two separately compiled kernels), and equal bits in bf16.

SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def masks_for(B, H, W, seed):
    """name -> [B,H,W] f32: soft random, binary, one with a row of zeros (the only row at B = 1), all ones"""
    g = gen(seed)
    soft = torch.rand(B, H, W, generator=g)
    zero_row = torch.rand(B, H, W, generator=g)
    zero_row[B // 2] = 0
    return dict(soft=soft, binary=(torch.rand(B, H, W, generator=g) > 0.5).float(), zero_row=zero_row, ones=torch.ones(B, H, W))


def levels64(m):
    out = [m.double()[:, None]]
    for _ in range(4):
        out.append(F.avg_pool2d(out[-1], 2))
    return [x[:, 0] for x in out]


@pytest.mark.parametrize("H,W", [(44, 44), (48, 40), (33, 70), (64, 64), (256, 256)])
def test_mask_pyramid_vs_float64(H, W):
    from dge_amd import ops
    worst = dict(level=0.0, inv_sum=0.0)
    for B in (1, 3):
        for name, m in masks_for(B, H, W, 7 * H + W + B).items():
            lev, inv, sums = ops.mask_pyramid(m.cuda())
            ref = levels64(m)
            assert [tuple(x.shape) for x in lev] == [(B, H >> k, W >> k) for k in range(5)] == [tuple(x.shape) for x in ref]
            assert torch.equal(lev[0].cpu(), m)
            for k in range(5):
                got = lev[k].cpu().double()
                top = float(ref[k].abs().max())
                err = float((got - ref[k]).abs().max()) / top if top > 0 else float((got != 0).any())
                worst["level"] = max(worst["level"], err)
                assert err <= ELEM_BOUND, (name, B, k, err)
                s = ref[k].sum(dim=(1, 2))
                for b in range(B):
                    if float(s[b]) == 0.0:
                        assert float(inv[b, k]) == 0.0 and float(sums[b, k]) == 0.0, (name, B, k, b)
                    else:
                        e = abs(float(inv[b, k]) * float(s[b]) - 1.0)
                        worst["inv_sum"] = max(worst["inv_sum"], e)
                        assert e <= INV_SUM_BOUND, (name, B, k, b, e)
                if name == "ones":
                    assert torch.equal(lev[k].cpu(), torch.ones(B, H >> k, W >> k))
                    hw = torch.tensor(float((H >> k) * (W >> k)), dtype=torch.float32)
                    assert torch.equal(inv[:, k].cpu(), (1.0 / hw).expand(B))
            if B > 1:          # a row alone has the bits it has in the batch
                for b in range(B):
                    l1, i1, s1 = ops.mask_pyramid(m[b:b + 1].cuda())
                    assert all(torch.equal(l1[k][0], lev[k][b]) for k in range(5)), (name, b)
                    assert torch.equal(i1[0], inv[b]) and torch.equal(s1[0], sums[b]), (name, b)
    meas(f"mask_pyramid.{H}x{W}", **worst)


def head_ref64(feat, lin, mk, inv, gscale):
    """float64 on the kernel's operands: (dist [B], g1 [B,1,HW,C]) of the weighted head with the weights mk * inv"""
    B = feat.shape[0] // 2
    fa, fb = feat[:B].double(), feat[B:].double().requires_grad_(True)
    na = fa / (fa.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    nb = fb / (fb.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    d = (((na - nb) ** 2) * lin.double()).sum(-1).reshape(B, -1)
    dist = (mk.double() * d).sum(1) * inv.double()
    (gscale * dist.sum()).backward()
    return dist.detach(), fb.grad


def head_masks(B, HW, seed):
    g = gen(seed)
    one = torch.zeros(B, HW)
    one[:, HW // 2] = 0.37
    zero_row = torch.rand(B, HW, generator=g)
    zero_row[B // 2] = 0
    return dict(soft=torch.rand(B, HW, generator=g), one_pixel=one, zero_row=zero_row, ones=torch.ones(B, HW))


def run_head_w(feat, lin, mk, inv5, tap, gscale):
    """the weighted head of one tap + the finaliser with the other four taps switched off (inv_sum 0) -> dist [B], g1"""
    from dge_amd import ops
    B, HW, Cc = feat.shape[0] // 2, feat.shape[2], feat.shape[3]
    n = ops.lpips_head_w_slots(HW, Cc, ops.dtype_of(feat))
    slots = torch.full((B * n,), float("nan"), device="cuda")          # nothing pre-zeroed: every slot is written
    g1 = torch.full((B, 1, HW, Cc), float("nan"), dtype=feat.dtype, device="cuda")
    ops.lpips_head_w(feat, lin, mk, inv5, tap, slots, g1, gscale)
    dist = torch.full((B,), float("nan"), device="cuda")
    ops.lpips_head_w_finalize(slots, [0] * 5, [n] * 5, inv5, dist)
    return dist, g1, n


@pytest.mark.parametrize("cd", ["f32", "bf16"])
@pytest.mark.parametrize("Cc", [64, 128, 256, 512])
def test_head_w_and_finalize_vs_float64(Cc, cd):
    from dge_amd import ops
    from dge_amd._lib import lib, check
    tdt = torch.float32 if cd == "f32" else torch.bfloat16
    ep = 4 if cd == "f32" else 8
    ppb = 32 * (64 // min(64, Cc // ep))          # a workgroup's pixel range (4 waves x 8 iterations x pixels per wave)
    worst = dict(g1=0.0, dist=0.0, ones_vs_head=0.0)
    ones_bits_equal = True
    was = ops.is_deterministic()
    try:
        for HW in (1, 6, 25, ppb + 3):
            for B in (1, 3):
                g = gen(Cc + HW + B)
                feat = torch.relu(torch.randn(2 * B, 1, HW, Cc, generator=g)).to(tdt)          # VGG taps sit behind a ReLU
                lin = torch.rand(Cc, generator=g) * 0.1
                gscale = 1.0 / B
                fd, ld = feat.cuda(), lin.cuda()
                for tap, (name, mk) in enumerate(head_masks(B, HW, Cc + HW).items()):
                    s = mk.double().sum(1)
                    inv = torch.where(s > 0, 1.0 / s, torch.zeros_like(s)).float()
                    inv5 = torch.zeros(B, 5)
                    inv5[:, tap] = inv
                    ops.set_deterministic(False)
                    dist, g1, n = run_head_w(fd, ld, mk.cuda(), inv5.cuda(), tap, gscale)
                    assert n == (2 if HW > ppb else 1)
                    ops.set_deterministic(True)
                    dist_d, g1_d, _ = run_head_w(fd, ld, mk.cuda(), inv5.cuda(), tap, gscale)
                    assert torch.equal(dist, dist_d) and torch.equal(g1, g1_d), (name, HW, B)          # both reduction modes: equal bits
                    ref_dist, ref_g1 = head_ref64(feat, lin, mk, inv, gscale)
                    got_g1, got_dist = g1.cpu().double(), dist.cpu().double()
                    top = float(ref_g1.abs().max())
                    if cd == "f32":
                        err = float((got_g1 - ref_g1).abs().max()) / top if top > 0 else float((got_g1 != 0).any())
                        assert err <= ELEM_BOUND, (name, HW, B, err)
                    else:          # one bf16 rounding of every element, plus the f32 bound
                        over = (got_g1 - ref_g1).abs() - (2.0 ** -8 * ref_g1.abs() + ELEM_BOUND * top)
                        assert float(over.max()) <= 0, (name, HW, B, float(over.max()))
                        err = float((got_g1 - ref_g1).abs().max()) / top if top > 0 else 0.0
                    worst["g1"] = max(worst["g1"], err)
                    for b in range(B):
                        if float(s[b]) == 0.0:
                            assert float(dist[b]) == 0.0 and not bool((g1[b] != 0).any()), (name, HW, B, b)
                        else:
                            e = abs(float(got_dist[b]) / float(ref_dist[b]) - 1.0)
                            worst["dist"] = max(worst["dist"], e)
                            assert e <= HEAD_DIST_BOUND, (name, HW, B, b, e)
                    if B > 1:          # a row alone has the bits it has in the batch
                        for b in range(B):
                            rows = torch.tensor([b, B + b])
                            d1, h1, _ = run_head_w(feat[rows].cuda(), ld, mk[b:b + 1].cuda(), inv5[b:b + 1].cuda(), tap, gscale)
                            assert torch.equal(d1[0], dist[b]) and torch.equal(h1[0], g1[b]), (name, HW, B, b)
                    if name == "ones":          # against the unweighted head
                        val = torch.zeros(B, device="cuda")
                        h0 = torch.empty_like(g1)
                        ops.set_deterministic(False)
                        check(lib().dge_lpips_head(ops._p(fd), ops._f32(ld), ops._p(val), ops._p(h0), B, HW, Cc, gscale, ops.dtype_of(fd),
                                                   ops._stream()), "dge_lpips_head")
                        e = float((h0.double() - g1.double()).abs().max()) / max(float(h0.double().abs().max()), 1e-300)
                        worst["ones_vs_head"] = max(worst["ones_vs_head"], e)
                        ones_bits_equal = ones_bits_equal and torch.equal(h0, g1)
                        assert e <= ELEM_BOUND, (HW, B, e)
    finally:
        ops.set_deterministic(was)
    meas(f"lpips_head_w.C{Cc}.{cd}", ones_bits_equal=str(ones_bits_equal), **worst)


def scaling():
    return (C.c_float * 3)(*SHIFT), (C.c_float * 3)(*SCALE)


@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_masked_prep_and_adjoint(cd):
    from dge_amd import ops
    from dge_amd._lib import lib, check
    tdt = torch.float32 if cd == "f32" else torch.bfloat16
    dt = ops.F32 if cd == "f32" else ops.BF16
    B, h, w, CP = 3, 23, 17, 16
    g = gen(31)
    img = torch.rand(B, 3, h, w, generator=g) * 2 - 1
    m = torch.rand(B, h, w, generator=g)
    m[:, :4] = 0
    m[:, -4:] = 1
    gx = torch.randn(B, h, w, CP, generator=g).to(tdt)
    shift, scale = scaling()
    sh = torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1)
    inv = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(SCALE, dtype=torch.float32)).view(1, 3, 1, 1)
    # ---- forward
    x = torch.full((B, h, w, CP), float("nan"), dtype=tdt, device="cuda")
    ops.lpips_prep_masked(img.cuda(), m.cuda(), x, shift, scale, CP)
    host = (((m[:, None] * img) - sh) * inv).permute(0, 2, 3, 1)
    if cd == "f32":
        assert torch.equal(x[..., :3].cpu(), host)
    else:
        assert torch.equal(x[..., :3].cpu(), host.to(tdt))
    assert not bool((x[..., 3:] != 0).any())
    x1, x0 = torch.empty_like(x), torch.empty_like(x)
    ops.lpips_prep_masked(img.cuda(), torch.ones(B, h, w, device="cuda"), x1, shift, scale, CP)
    check(lib().dge_lpips_prep(ops._f32(img.cuda()), ops._p(x0), B, h * w, CP, shift, scale, dt, ops._stream()), "dge_lpips_prep")
    assert torch.equal(x1, x0)
    # ---- adjoint, written and accumulated
    prev = torch.randn(B, 3, h, w, generator=g)
    host_g = ((gx[..., :3].float().permute(0, 3, 1, 2) * inv) * 0.5) * m[:, None]
    for acc in (False, True):
        out = prev.clone().cuda() if acc else torch.full((B, 3, h, w), float("nan"), device="cuda")
        ops.lpips_prep_bwd_masked(gx.cuda(), m.cuda(), out, scale, CP, factor=0.5, accumulate=acc)
        assert torch.equal(out.cpu(), prev + host_g if acc else host_g), acc
        o1 = prev.clone().cuda() if acc else torch.empty((B, 3, h, w), device="cuda")
        o0 = o1.clone()
        ops.lpips_prep_bwd_masked(gx.cuda(), torch.ones(B, h, w, device="cuda"), o1, scale, CP, factor=0.5, accumulate=acc)
        check(lib().dge_lpips_prep_bwd(ops._p(gx.cuda()), ops._f32(o0), B, h * w, CP, scale, 0.5, 1 if acc else 0, dt, ops._stream()),
              "dge_lpips_prep_bwd")
        assert torch.equal(o1, o0), acc
    assert not bool((host_g[:, :, :4] != 0).any())


@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (3, 3, 64, 48)])
def test_mask_blend_has_the_bits_of_the_host_formula(shape):
    from dge_amd import ops
    B, _, H, W = shape
    g = gen(B + H)
    a, b = torch.rand(shape, generator=g) * 2 - 1, torch.rand(shape, generator=g) * 2 - 1
    m = torch.rand(B, 1, H, W, generator=g)
    m[:, :, 0] = 0
    m[:, :, -1] = 1
    out = ops.mask_blend(m.cuda(), a.cuda(), b.cuda())
    assert torch.equal(out.cpu(), m * a + (1 - m) * b)
    assert torch.equal(out[:, :, 0].cpu(), b[:, :, 0]) and torch.equal(out[:, :, -1].cpu(), a[:, :, -1])
