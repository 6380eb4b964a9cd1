"""E_BIG backward with an image gradient and in its frozen form (autograd_encbig.big_encoder_backward need_img / params):
g_img and every parameter gradient against the reference's autograd (tests/golden/encbig_imggrad.npz, tools/gen_golden_embed_big.py),
the frozen form's launches and bits, and the default call's launch sequence against a restatement of what it issued before the
image gradient was added."""
import numpy as np
import pytest
import torch

from tests.conftest import golden, meas, with_fixture_params
from tests.golden import recipe as R

pytestmark = pytest.mark.gpu


def _l2rel(a, b):
    a = a.detach().float().cpu().flatten(); b = torch.as_tensor(np.asarray(b)).float().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _cos(a, b):
    a = a.detach().float().cpu().flatten(); b = torch.as_tensor(np.asarray(b)).float().flatten()
    return torch.nn.functional.cosine_similarity(a, b, dim=0).item()


def _relerr(a, b):
    a = a.detach().float().cpu(); b = torch.as_tensor(np.asarray(b)).float()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _model(cd, g):
    from dge_amd.encoder_variants import BigBE
    E = BigBE(startf=32, maxf=512, layer_count=5, biggan=True, compute_dtype=cd).cuda()
    E.load_state_dict(with_fixture_params(R.fill_encbig({n: list(v.shape) for n, v in E.state_dict().items()}, 81), g))
    E.train()
    return E


def _inputs():
    g0 = golden("encbig_small.npz")
    noises = [R.randn(f"ebg.noise{i}", tuple(s), 81).cuda() for i, s in enumerate(g0["noise_shapes"].tolist())]
    return R.randn("ebg.img", (2, 3, 64, 64), 81, 0.5).cuda(), R.randn("ebg.cond", (2, 256), 81, 0.5).cuda(), noises


def _check_param_grads(named_grads, g, tol, min_checked, global_tol=None, skip_tiny=1e-3, tiny_abs=5e-2):
    """test_encvar._check_grads for a fixture that stores the first 4096 elements (and the norm) of every larger gradient."""
    pairs = []
    for k, gr in named_grads.items():
        if "grad:" + k not in g.files:
            assert gr is None or float(gr.abs().max()) == 0.0, k
            continue
        ref, nrm = torch.as_tensor(g["grad:" + k]).float(), float(g["norm:" + k])
        mine = gr.detach().float().cpu()
        if nrm < skip_tiny:
            assert float(mine.norm()) < tiny_abs, (k, float(mine.norm()))
            continue
        pairs.append((k, mine, ref, nrm))
    worst = max((_l2rel(m if m.numel() <= 4096 else m.flatten()[:4096], r), k) for k, m, r, _ in pairs)
    a = torch.cat([(m if m.numel() <= 4096 else m.flatten()[:4096]).flatten() for _, m, _, _ in pairs])
    b = torch.cat([r.flatten() for _, _, r, _ in pairs])
    gl2, gcos = ((a - b).norm() / b.norm()).item(), torch.nn.functional.cosine_similarity(a, b, dim=0).item()
    meas("encbig_imggrad_params", tol=tol, worst_l2=worst[0], key=worst[1], global_l2=gl2, global_cos=gcos)
    for k, mine, ref, nrm in pairs:
        assert abs(float(mine.norm()) - nrm) < tol * nrm + 1e-6, (k, float(mine.norm()), nrm)
        assert _l2rel(mine if mine.numel() <= 4096 else mine.flatten()[:4096], ref) < tol, k
    assert len(pairs) >= min_checked, len(pairs)
    if global_tol is not None:
        assert gl2 < global_tol[0] and gcos > global_tol[1], (gl2, gcos)


@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_e_big_image_gradient_vs_reference_golden(cd):
    """E_BIG with img.requires_grad_(True), train mode, gradients entering through both outputs: g_img and every parameter gradient
    against the reference's autograd.  Parameter bounds: those of test_encvar.test_hip_e_big_gradients_vs_reference_golden.
    g_img, deterministic run: f32 measured L2 G_IMG_F32_MEASURED (bound 3x); bf16 measured L2 / cosine G_IMG_BF16_MEASURED
    (bounds 1.5x the L2 and the cosine's distance from 1, as the E_Blur sibling sets them)."""
    g = golden("encbig_imggrad.npz")
    assert float(g["kink_margin"]) > 1e-4
    E = _model(cd, g)
    img, cond, noises = _inputs()
    img.requires_grad_(True)
    c_v, z = E(img, cond, noises=noises)
    tol = 3e-4 if cd == "f32" else 5e-2
    assert _relerr(c_v, g["c_v"]) < tol and _relerr(z, g["z"]) < tol
    loss = (z * R.randn("ebg.gz", tuple(z.shape), 82).cuda()).sum() + (c_v * R.randn("ebg.gcv", tuple(c_v.shape), 82).cuda()).sum()
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) < (2e-5 if cd == "f32" else 1e-3) * abs(float(g["loss"]))
    assert img.grad is not None and img.grad.shape == img.shape and img.grad.dtype == torch.float32
    l2, cos = _l2rel(img.grad, g["g_img"]), _cos(img.grad, g["g_img"])
    meas("encbig_img_grad", cd=cd, img_l2=l2, img_cos=cos)
    named = {k: p.grad for k, p in E.named_parameters()}
    if cd == "f32":
        _check_param_grads(named, g, 1e-4, 60)
        assert l2 < G_IMG_F32_BOUND, l2
    else:
        _check_param_grads(named, g, 0.2, 60, global_tol=(0.085, 0.9975))
        assert l2 < G_IMG_BF16_BOUND[0] and cos > G_IMG_BF16_BOUND[1], (l2, cos)


# g_img against the reference, measured on MI355X in deterministic mode (MEAS encbig_img_grad)
G_IMG_F32_MEASURED = 1.74e-6                    # relative L2
G_IMG_F32_BOUND = 5e-6                          # <= 3x the measured value
G_IMG_BF16_MEASURED = (0.0858, 0.99632)         # relative L2, cosine (leaky-relu slopes flipped by bf16 storage rounding, as in its siblings)
G_IMG_BF16_BOUND = (0.129, 0.9945)              # 1.5x the L2, 1.5x the cosine's distance from 1


# ------------------------------------------------------------------ launch traces
_TRACED = ("act_bwd", "in_bwd", "conv_wgrad", "conv2d", "chan_sum", "dense_wgrad", "linear_t", "fromrgb_bwd", "fromrgb_dgrad",
           "affine_bwd_fromrgb_img", "nchw_to_nhwc", "scale_")


def _trace(monkeypatch):
    """Every call of the ops the E_BIG backward is made of, as (op, its arguments: shape and dtype of a tensor, the value of a
    scalar) in call order; the grouped conditional-batch-norm launch is recorded by its caller's name."""
    from dge_amd import autograd_encbig, ops
    calls = []

    def sig(v):
        if torch.is_tensor(v):
            return (tuple(v.shape), str(v.dtype))
        if isinstance(v, (bool, int, float, str, type(None))):
            return v
        if isinstance(v, (list, tuple)):
            return tuple(sig(x) for x in v)
        return type(v).__name__

    def wrap(mod, name, tag):
        orig = getattr(mod, name)

        def f(*a, **kw):
            calls.append((tag, tuple(sig(v) for v in a), tuple(sorted((k, sig(v)) for k, v in kw.items()))))
            return orig(*a, **kw)
        monkeypatch.setattr(mod, name, f)
    for name in _TRACED:
        wrap(ops, name, name)
    wrap(autograd_encbig, "_cbn_param_grads_flush", "cbn_sn_wgrad_group")
    return calls


def _saved_forward(E, img, cond, noises):
    from dge_amd.autograd_encbig import big_encoder_forward
    _, c_v, z, saved = big_encoder_forward(E, img, cond, noises, save=True)
    return saved, R.randn("ebg.gz", tuple(z.shape), 82).cuda(), R.randn("ebg.gcv", tuple(c_v.shape), 82).cuda()


def _backward_as_before(E, saved, g_z, g_cv):
    """What big_encoder_backward(E, saved, g_z, g_cv) issued before it learnt need_img / params: the same ops, in that order."""
    from dge_amd import ops
    from dge_amd.autograd_encbig import _affine_coef, _cbn_param_grads, _cbn_param_grads_flush
    from dge_amd.enc_steps import blocks, conv_bwd, fromrgb_param_grads, grads_in_order, linear_backward, red_param_grads
    from dge_amd.weight_cache import pack_cache
    cache = pack_cache(E)
    dev = g_z.device
    B = g_z.shape[0]
    Rr = saved["img"].shape[2]
    dt = ops.dtype_of(saved["x0"])
    cond = saved["cond"]
    grads, pend = {}, []
    g_cvt = linear_backward(E.new_final_2, g_z.float().contiguous(), saved["c_v"], grads, "new_final_2")
    g_cvt = g_cvt + g_cv.float()
    g_flat = linear_backward(E.new_final_1, g_cvt.contiguous(), saved["flat"], grads, "new_final_1")
    L = len(saved["blocks"])
    C_last = E.decode_block[L - 1].inputs
    g_out = ops.nchw_to_nhwc(g_flat.view(B, C_last, Rr >> (L - 1), Rr >> (L - 1)), B, dt)
    for j, blk, rec, pre, Cc, C2, H, _ in blocks(E, Rr, saved):
        x, x1 = rec["x"], rec["x1"]
        red1 = ops.zeros((Cc, 2), dev)
        extra, extra_pool, extra_scale = None, False, 1.0
        if blk.has_second_conv:
            has3 = Cc != C2
            red2 = ops.zeros((C2, 2), dev)
            g_pre2 = ops.act_bwd(g_out, rec["x2"], rec["n2"], pool=True, scale=0.25, red=red2, slope=0.04 if has3 else 0.2)
            red_param_grads(grads, pre, 2, red2)
            g_u2, dots2 = conv_bwd(cache, grads, pre + "conv_2", blk.conv_2, g_pre2, x1, dt, H, rec["a2"], rec["b2"])
            _cbn_param_grads(blk.batch_norm_2, rec["c2"], dots2, cond, grads, pre + "batch_norm_2", pend)
            g_pre1 = ops.in_bwd(g_u2, x1, _affine_coef(rec["a2"]), noise=rec["n1"], act=True, red=red1)
            if has3:
                xp = rec["xp"]
                grads[pre + "conv_3.bias"] = ops.chan_sum(g_out)
                g_u3, dots3 = conv_bwd(cache, grads, pre + "conv_3", blk.conv_3, g_out, xp, dt, None, rec["a3"], rec["b3"])
                _cbn_param_grads(blk.batch_norm_3, rec["c3"], dots3, cond, grads, pre + "batch_norm_3", pend)
                extra = ops.in_bwd(g_u3, xp, _affine_coef(rec["a3"]))
            else:
                extra = g_out
            extra_pool, extra_scale = True, 0.25
        else:
            g_pre1 = ops.act_bwd(g_out, x1, rec["n1"], pool=False, scale=1.0, red=red1)
        red_param_grads(grads, pre, 1, red1)
        g_u1, dots1 = conv_bwd(cache, grads, pre + "conv_1", blk.conv_1, g_pre1, x, dt, H, rec["a1"], rec["b1"])
        _cbn_param_grads(blk.batch_norm_1, rec["c1"], dots1, cond, grads, pre + "batch_norm_1", pend)
        g_out = ops.in_bwd(g_u1, x, _affine_coef(rec["a1"]), extra=extra, extra_pool=extra_pool, extra_scale=extra_scale)
    _cbn_param_grads_flush(pend, cond, grads)
    fromrgb_param_grads(E, saved, g_out, grads)
    return grads_in_order(E, grads)


@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_default_backward_issues_the_launches_it_issued_before(cd, monkeypatch):
    """Detached image, trained encoder (what E_align_s2 --mtype 4 runs): the traced op sequence and the KERNEL_LOG sequence of
    big_encoder_backward equal those of the restatement above, and so do the gradients (deterministic mode: to the bit)."""
    from dge_amd import ops
    from dge_amd.autograd_encbig import big_encoder_backward
    g = golden("encbig_imggrad.npz")
    E = _model(cd, g)
    img, cond, noises = _inputs()
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        with torch.no_grad():
            saved, g_z, g_cv = _saved_forward(E, img, cond, noises)
            calls = _trace(monkeypatch)
            runs = []
            for fn in (big_encoder_backward, _backward_as_before):
                del calls[:]
                ops.KERNEL_LOG = log = []
                try:
                    out = fn(E, saved, g_z, g_cv)
                finally:
                    ops.KERNEL_LOG = None
                torch.cuda.synchronize()
                runs.append((list(calls), [n for n, _ in log], out))
    finally:
        ops.set_deterministic(was)
    (calls_a, log_a, out_a), (calls_b, log_b, out_b) = runs
    assert len(calls_a) > 40 and calls_a == calls_b
    assert log_a == log_b
    assert "affine_bwd_fromrgb_img" not in [c[0] for c in calls_a] and "fromrgb_bwd" in [c[0] for c in calls_a]
    assert len(out_a) == len(out_b)
    for ga, gb in zip(out_a, out_b):
        assert (ga is None) == (gb is None)
        if ga is not None:
            assert torch.equal(ga, gb)


@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_frozen_backward_launches_no_parameter_gradient_and_keeps_the_bits(cd, monkeypatch):
    """params=False: no weight-gradient, reduction, conditional-batch-norm, FromRGB-reduction or head-weight-gradient launch, every
    parameter gradient None, and g_img equal to the trained form's to the bit (deterministic mode).  The autograd function takes
    this form for an encoder whose parameters are frozen."""
    from dge_amd import ops
    from dge_amd.autograd_encbig import big_encoder_backward
    g = golden("encbig_imggrad.npz")
    E = _model(cd, g)
    img, cond, noises = _inputs()
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        with torch.no_grad():
            saved, g_z, g_cv = _saved_forward(E, img, cond, noises)
            grads_t, g_img_t = big_encoder_backward(E, saved, g_z, g_cv, need_img=True)
            calls = _trace(monkeypatch)
            ops.KERNEL_LOG = log = []
            try:
                grads_f, g_img_f = big_encoder_backward(E, saved, g_z, g_cv, need_img=True, params=False)
            finally:
                ops.KERNEL_LOG = None
            torch.cuda.synchronize()
        names = [n for n, _ in log]
        opsrun = [c[0] for c in calls]
        for bad in ("conv_wgrad", "dense_wgrad", "fromrgb_bwd", "chan_sum", "cbn_sn_wgrad_group", "scale_"):
            assert bad not in opsrun, (bad, opsrun)
        for n in names:
            assert "wgrad" not in n and "cbn_sn_wgrad" not in n and "fromrgb_bwd" not in n and not n.endswith(",fr>"), n
        tag = "bf16" if cd == "bf16" else "f32"
        assert names.count(f"affine_bwd_fromrgb_img<{tag},data>") == 1, names
        assert all(x is None for x in grads_f) and any(x is not None for x in grads_t)
        assert g_img_f.shape == (2, 3, 64, 64) and torch.equal(g_img_f, g_img_t)
        # through autograd: frozen parameters select the same form
        # (a fresh model: every train-mode forward runs a power iteration on the spectral-norm buffers)
        monkeypatch.undo()
        E2 = _model(cd, g)
        for p in E2.parameters():
            p.requires_grad_(False)
        x = img.clone().requires_grad_(True)
        c_v, z = E2(x, cond, noises=noises)
        torch.autograd.backward([c_v, z], [g_cv, g_z])
        assert all(p.grad is None for p in E2.parameters())
        assert torch.equal(x.grad, g_img_t)
    finally:
        ops.set_deterministic(was)


def test_condition_vector_gradient_stays_refused():
    from dge_amd import ops
    g = golden("encbig_imggrad.npz")
    E = _model("f32", g)
    img, cond, noises = _inputs()
    with pytest.raises(ops.DgeError, match="condition vector"):
        E(img, cond.requires_grad_(True), noises=noises)


def test_unsupported_channel_count_takes_the_composed_passes(monkeypatch):
    """Where the kernel refuses the channel count the backward falls back to in_bwd -> fromrgb_dgrad -> fromrgb_bwd, with the same
    result up to the rounding of the stored gradient (f32: summation order only)."""
    from dge_amd import autograd_encbig, ops
    g = golden("encbig_imggrad.npz")
    E = _model("f32", g)
    img, cond, noises = _inputs()
    with torch.no_grad():
        saved, g_z, g_cv = _saved_forward(E, img, cond, noises)
        grads_a, g_img_a = autograd_encbig.big_encoder_backward(E, saved, g_z, g_cv, need_img=True)
        monkeypatch.setattr(ops, "affine_bwd_fromrgb_img_supported", lambda Cc, dt: False)

        def boom(*a, **kw):
            raise AssertionError("fused launch used for a refused channel count")
        monkeypatch.setattr(ops, "affine_bwd_fromrgb_img", boom)
        grads_b, g_img_b = autograd_encbig.big_encoder_backward(E, saved, g_z, g_cv, need_img=True)
    assert _l2rel(g_img_b, g_img_a.cpu().numpy()) < 1e-5
    names = [n for n, _ in E.named_parameters()]
    for n, a, b in zip(names, grads_a, grads_b):
        if n.startswith("FromRGB"):
            assert _l2rel(b, a.cpu().numpy()) < 1e-5, n
