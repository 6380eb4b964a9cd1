"""Per-sample forms of the loss kernels (losses.image_loss_tsa_rows / space_loss_rows, ops.latent_pnorm_rows): every sample of a
batch against the oracle's autograd on that sample alone.  The rows of `b` are scaled differently (a*(0.8 - 0.25*r) + noise), so
the per-sample losses lie far apart and far from the loss of the coupled batch: a result that couples the rows cannot pass."""
import functools

import pytest
import torch

from tests.golden import recipe as R
from oracle import ref_torch as O

pytestmark = pytest.mark.gpu
WEIGHTS = (1.0, 0.375, 0.625)
INFO_KEYS = ("mse", "mse_mean", "mse_std", "kl", "cos", "ssim", "lpips")
# (3, 3, 44, 30): width no multiple of 4 -> the scalar forms, two reduction blocks per sample.
# (2, 3, 320, 256): the 16-byte forms, pooling factor 2 on the first two windows, a 220 x 176 third window (no multiple of the
# 16 x 16 SSIM tile), 80 reduction blocks per sample.
SHAPES = [(3, 3, 44, 30), (2, 3, 320, 256)]


def _scaled_rows(a, noise):
    s = torch.tensor([0.8 - 0.25 * r for r in range(a.shape[0])]).view(-1, *([1] * (a.dim() - 1)))
    return a * s + noise


@functools.lru_cache(maxsize=None)
def tsa_case(shape):
    """(a, b, per-sample oracle loss, oracle gradient [B,...], per-sample per-window oracle terms, coupled oracle loss)"""
    a = R.randn("tsa.a", shape, 3, 0.4)
    b = _scaled_rows(a, R.randn("tsa.b", shape, 3, 0.2))
    zero_lp = lambda x, y: torch.zeros(x.shape[0], 1, 1, 1)

    def tsa(x1, x2):
        tot, terms = 0, []
        for wgt, (c1, c2) in zip(WEIGHTS, zip([x1, *O.attention_crops(x1)], [x2, *O.attention_crops(x2)])):
            l, d = O.space_loss(c1, c2, lpips_fn=zero_lp)
            tot = tot + wgt * l
            terms.append([float(l.detach())] + [float(d[k].detach()) for k in INFO_KEYS])
        return tot, terms
    losses, grads, infos = [], [], []
    for r in range(shape[0]):
        br = b[r:r + 1].clone().requires_grad_(True)
        tot, terms = tsa(a[r:r + 1], br)
        tot.backward()
        losses.append(float(tot.detach())); grads.append(br.grad); infos.append(terms)
    with torch.no_grad():
        coupled = float(tsa(a, b)[0])
    return a, b, losses, torch.cat(grads), torch.tensor(infos), coupled


def _check_info(got, ref, where):
    # the bound test_loss_gpu.py applies to the logged terms of the same kernels' arithmetic
    for i in range(1, 8):
        assert abs(got[i] - ref[i]) <= 5e-4 * abs(ref[i]) + 2e-6, (where, i, float(got[i]), float(ref[i]))


@pytest.mark.parametrize("shape", SHAPES, ids=["scalar", "vec4"])
def test_image_loss_tsa_rows_vs_oracle_per_row(shape):
    from dge_amd import losses, ops
    a, b, ref_loss, ref_grad, ref_info, coupled = tsa_case(shape)
    B = shape[0]
    assert all(abs(l - coupled) > 0.1 * coupled for l in ref_loss[::B - 1]), (ref_loss, coupled)     # the rows are told apart
    was = ops.is_deterministic()
    res = {}
    try:
        for det in (False, True):
            ops.set_deterministic(det)
            bg = b.cuda().requires_grad_(True)
            log = []
            ops.KERNEL_LOG = log
            try:
                loss, info = losses.image_loss_tsa_rows(a.cuda(), bg, None, WEIGHTS, (True, True, True))
                loss.backward()
            finally:
                ops.KERNEL_LOG = None
            torch.cuda.synchronize()
            res[det] = (loss.detach().cpu(), info.cpu(), bg.grad.cpu(), [n for n, _ in log])
    finally:
        ops.set_deterministic(was)
    loss, info, grad, names = res[False]
    vec = shape[3] % 4 == 0
    assert names == ["loss_reduce_rows_c3v4" if vec else "loss_reduce_rows", "ssim_fwd_rows", "ssim_fwd_rows", "ssim_fwd_rows",
                     "space_loss_finalize_rows", "space_loss_bwd_rows_v4" if vec else "space_loss_bwd_rows"], names
    assert tuple(info.shape) == (B, 3, 8)
    got_rows = info[:, 0, 0] * WEIGHTS[0] + info[:, 1, 0] * WEIGHTS[1] + info[:, 2, 0] * WEIGHTS[2]
    for r in range(B):
        e_l = abs(float(got_rows[r]) - ref_loss[r]) / abs(ref_loss[r])
        e_g = ((grad[r] - ref_grad[r]).abs().max() / ref_grad[r].abs().max()).item()
        print("MEAS tsa_rows", shape, r, float(got_rows[r]), ref_loss[r], e_l, e_g)
        assert e_l < 2e-4, (r, float(got_rows[r]), ref_loss[r])
        assert e_g < 2e-3, (r, e_g)
        for k in range(3):
            assert abs(float(info[r, k, 0]) - float(ref_info[r, k, 0])) < 2e-4 * abs(float(ref_info[r, k, 0])), (r, k)
            _check_info(info[r, k], ref_info[r, k], (r, k))
    assert abs(float(loss) - sum(ref_loss)) < 2e-4 * sum(ref_loss)
    # no atomics and no mode-dependent path: the deterministic mode runs the same kernels and gives the same bits
    assert res[True][3] == names
    for x, y in zip(res[False][:3], res[True][:3]):
        assert torch.equal(x, y)


@functools.lru_cache(maxsize=None)
def latent_case():
    w1 = R.randn("loss.w1", (3, 10, 512), 2)
    w2 = _scaled_rows(w1, R.randn("loss.w2", (3, 10, 512), 2, 0.3))
    losses, g1, g2, infos = [], [], [], []
    for r in range(3):
        x1 = w1[r:r + 1].clone().requires_grad_(True)
        x2 = w2[r:r + 1].clone().requires_grad_(True)
        l, d = O.space_loss(x1, x2, image_space=False)
        l.backward()
        losses.append(float(l.detach())); g1.append(x1.grad); g2.append(x2.grad)
        infos.append([float(l.detach())] + [float(d[k].detach()) for k in INFO_KEYS])
    with torch.no_grad():
        coupled = float(O.space_loss(w1, w2, image_space=False)[0])
    return w1, w2, losses, torch.cat(g1), torch.cat(g2), torch.tensor(infos), coupled


def test_space_loss_rows_on_latents_vs_oracle_per_row():
    from dge_amd import losses
    w1, w2, ref_loss, ref_g1, ref_g2, ref_info, coupled = latent_case()
    assert abs(ref_loss[0] - coupled) > 0.1 * coupled and abs(ref_loss[2] - coupled) > 0.1 * coupled, (ref_loss, coupled)
    x1 = w1.cuda().requires_grad_(True)
    x2 = w2.cuda().requires_grad_(True)
    loss, info = losses.space_loss_rows(x1, x2, image_space=False)
    loss.backward()
    info = info.cpu()
    assert tuple(info.shape) == (3, 8)
    for r in range(3):
        e_l = abs(float(info[r, 0]) - ref_loss[r]) / ref_loss[r]
        e1 = ((x1.grad[r].cpu() - ref_g1[r]).abs().max() / ref_g1[r].abs().max()).item()
        e2 = ((x2.grad[r].cpu() - ref_g2[r]).abs().max() / ref_g2[r].abs().max()).item()
        print("MEAS latent_rows", r, float(info[r, 0]), ref_loss[r], e_l, e1, e2)
        assert e_l < 2e-4 and e1 < 2e-3 and e2 < 2e-3, (r, e_l, e1, e2)
        _check_info(info[r], ref_info[r], r)
    assert abs(float(loss.detach()) - sum(ref_loss)) < 2e-4 * sum(ref_loss)
    # only the second argument carries a gradient: the same numbers, nothing for the first
    y2 = w2.cuda().requires_grad_(True)
    loss_b, _ = losses.space_loss_rows(w1.cuda(), y2, image_space=False)
    loss_b.backward()
    assert torch.equal(loss_b.detach(), loss.detach()) and torch.equal(y2.grad, x2.grad)
    with pytest.raises(ValueError):
        losses.space_loss_rows(x1, x2, global_batch=losses.GlobalBatch(2))
    with pytest.raises(ValueError):
        losses.image_loss_tsa_rows(torch.zeros(1, 3, 8, 8).cuda(), torch.zeros(1, 3, 8, 8).cuda(), global_batch=losses.GlobalBatch(2))


def test_space_loss_rows_const_term_equals_one_row_slices():
    """[3, 64, 4, 4]: the StyleGAN1 const term; every sample against the coupled space_loss on its one-row slice."""
    from dge_amd import losses
    c2 = R.randn("rows.c2", (3, 64, 4, 4), 4).cuda()
    c3 = _scaled_rows(c2.cpu(), R.randn("rows.c3", (3, 64, 4, 4), 4, 0.3)).cuda().requires_grad_(True)
    loss, info = losses.space_loss_rows(c2, c3, image_space=False)
    loss.backward()
    tot = 0.0
    for r in range(3):
        y = c3.detach()[r:r + 1].clone().requires_grad_(True)
        l, i8 = losses.space_loss(c2[r:r + 1], y, image_space=False)
        l.backward()
        tot += float(l)
        assert abs(float(info[r, 0]) - float(l)) < 2e-4 * float(l), (r, float(info[r, 0]), float(l))
        _check_info(info[r].cpu(), i8.cpu(), r)
        assert ((c3.grad[r:r + 1] - y.grad).abs().max() / y.grad.abs().max()).item() < 2e-3
    assert abs(float(loss) - tot) < 2e-4 * tot
    assert abs(float(info[0, 0]) - float(info[2, 0])) > 0.5 * float(info[0, 0])


@pytest.mark.parametrize("p", [1, 2, 3])
def test_latent_pnorm_rows_kernel_matches_torch(p):
    from dge_amd import ops
    shape = (3, 10, 512)
    w = R.randn(f"pnorm.{p}.{shape}", shape, 9) * torch.tensor([1.0, 0.5, 2.0]).view(3, 1, 1)
    wd = w.double().requires_grad_(True)
    ref = torch.linalg.vector_norm(wd.reshape(3, -1), ord=p, dim=1)
    ref.sum().backward()
    wc = w.cuda()
    l2 = torch.empty(3, dtype=torch.float32, device="cuda")
    n = ops.latent_pnorm_rows(wc, p, out_l2=l2)
    ref_l2 = torch.linalg.vector_norm(w.double().reshape(3, -1), dim=1)
    gout = torch.tensor([1.0, 2.0, 0.5], device="cuda")
    g = torch.ones_like(wc)
    ops.latent_pnorm_rows_bwd(wc, n, g, p, beta=0.5, gout=gout)
    for r in range(3):
        assert abs(float(n[r]) - float(ref[r])) <= 1e-6 * float(ref[r]), (r, float(n[r]), float(ref[r]))
        assert abs(float(l2[r]) - float(ref_l2[r])) <= 1e-6 * float(ref_l2[r])
        want = 1.0 + 0.5 * float(gout[r]) * wd.grad[r]
        assert ((g[r].double().cpu() - want).abs().max() / want.abs().max()).item() < 1e-6, r
    assert torch.equal(ops.latent_l2_rows(wc), l2)
    # a zero row: zero gradient, and the neighbours' gradients are what they are without it
    wz = wc.clone()
    wz[1] = 0.0
    nz = ops.latent_pnorm_rows(wz, p)
    gz = torch.zeros_like(wz)
    ops.latent_pnorm_rows_bwd(wz, nz, gz, p, beta=1.0)
    g0 = torch.zeros_like(wc)
    ops.latent_pnorm_rows_bwd(wc, n, g0, p, beta=1.0)
    assert float(nz[1]) == 0.0 and torch.isfinite(gz).all() and float(gz[1].abs().max()) == 0.0
    assert torch.equal(gz[0], g0[0]) and torch.equal(gz[2], g0[2]) and torch.equal(nz[[0, 2]], n[[0, 2]])
