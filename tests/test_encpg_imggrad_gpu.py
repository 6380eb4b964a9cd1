"""E_PG backward with an image gradient and in its frozen form (autograd_encpg.pg_encoder_backward need_img / params): g_img and
every parameter gradient against the reference's autograd (tests/golden/encpg_imggrad.npz, tools/gen_golden_embed_pg.py), the
frozen form's launches and bits, and the default call's launch sequence against a restatement of what it issued before the image
gradient was added."""
import pytest
import torch

from tests.conftest import golden, meas, with_fixture_params
from tests.golden import recipe as R
from tests.test_encbig_imggrad_gpu import _check_param_grads, _cos, _l2rel
from tests.test_encvar import pg_params

pytestmark = pytest.mark.gpu


def _model(cd, g):
    from dge_amd.encoder_variants import PGBE
    E = PGBE(startf=32, maxf=512, layer_count=5, pggan=True, compute_dtype=cd).cuda()
    E.load_state_dict(with_fixture_params(pg_params(E), g))
    return E


def _inputs():
    g0 = golden("encpg_small.npz")
    noises = [R.randn(f"ep.noise{i}", tuple(s), 62).cuda() for i, s in enumerate(g0["noise_shapes"].tolist())]
    return R.randn("ep.img", (2, 3, 64, 64), 62, 0.5).cuda(), noises


def _run(cd, det):
    from dge_amd import ops
    g = golden("encpg_imggrad.npz")
    E = _model(cd, g)
    img, noises = _inputs()
    img.requires_grad_(True)
    was = ops.is_deterministic()
    ops.set_deterministic(det)
    try:
        _, z = E(img, noises=noises)
        loss = (z * R.randn("ep.gz", tuple(z.shape), 64).cuda()).sum()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    return g, E, img, z, loss


@pytest.mark.parametrize("det", [True, pytest.param(False, marks=pytest.mark.nondet)], ids=["deterministic", "atomics"])
def test_e_pg_image_gradient_f32_vs_reference_golden(det):
    """f32, img.requires_grad_(True): g_img (relative L2) and every parameter gradient within 1e-4 of the reference's autograd, the
    project's f32 bound for E_PG gradients (test_encvar.test_hip_e_pg_gradients_vs_reference_golden), in the deterministic and
    in the default (atomics) reduction mode.  The fixture keeps every leaky-relu pre-activation, FromRGB's included, off the kink."""
    g, E, img, z, loss = _run("f32", det)
    assert float(g["kink_margin"]) > 1e-4
    assert _l2rel(z, g["z"]) < 3e-4
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-5 * abs(float(g["loss"]))
    assert img.grad is not None and img.grad.shape == img.shape and img.grad.dtype == torch.float32
    l2 = _l2rel(img.grad, g["g_img"])
    meas("encpg_img_grad", cd="f32", det=float(det), img_l2=l2, img_cos=_cos(img.grad, g["g_img"]))
    assert l2 < 1e-4, l2
    _check_param_grads({k: p.grad for k, p in E.named_parameters()}, g, 1e-4, 40)


# g_img and the parameter gradients against the reference in bf16, measured on MI355X in deterministic mode (MEAS encpg_img_grad
# and encbig_imggrad_params, the name the helper shared with test_encbig_imggrad_gpu prints under): bf16 storage rounding (2^-9
# relative) is 40x the fixture's kink margin, so leaky-relu slopes flip against the f32 reference, as in test_encvar's bf16 case.
# The bounds are 1.5x the measured values (the cosine: 1.5x its distance from 1).
G_IMG_BF16_MEASURED = (0.1668, 0.98607)         # relative L2, cosine
G_IMG_BF16_BOUND = (0.25, 0.9791)
PARAMS_BF16_MEASURED = (0.2254, 0.1579, 0.98750)     # worst tensor L2 (decode_block.1.bias_1), all tensors as one vector: L2, cosine
PARAMS_BF16_BOUND = (0.338, 0.237, 0.9812)


def test_e_pg_image_gradient_bf16_vs_reference_golden():
    """bf16, deterministic: g_img and the parameter gradients within 1.5x the values this run gives (above), as
    test_encvar.test_hip_e_pg_gradients_vs_reference_golden sets its bf16 bounds."""
    g, E, img, z, loss = _run("bf16", True)
    assert _l2rel(z, g["z"]) < 5e-2
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-2 * abs(float(g["loss"]))
    l2, cos = _l2rel(img.grad, g["g_img"]), _cos(img.grad, g["g_img"])
    meas("encpg_img_grad", cd="bf16", det=1.0, img_l2=l2, img_cos=cos)
    _check_param_grads({k: p.grad for k, p in E.named_parameters()}, g, PARAMS_BF16_BOUND[0], 40, global_tol=PARAMS_BF16_BOUND[1:], tiny_abs=0.5)
    assert l2 < G_IMG_BF16_BOUND[0] and cos > G_IMG_BF16_BOUND[1], (l2, cos)


# ------------------------------------------------------------------ launch traces
_TRACED = ("act_bwd", "in_bwd", "in_bwd_coef", "conv_wgrad", "conv2d", "chan_sum", "dense_wgrad", "linear_t", "fromrgb_bwd", "fromrgb_dgrad",
           "in_bwd_fromrgb_img", "nchw_to_nhwc", "sg1_in_bwd_coef", "dot_stats", "_sum_over_batch")


def _trace(monkeypatch):
    """Every call of the ops the E_PG backward is made of, as (op, its arguments: shape and dtype of a tensor, the value of a
    scalar), in call order."""
    from dge_amd import ops
    calls = []

    def sig(v):
        if torch.is_tensor(v):
            return (tuple(v.shape), str(v.dtype))
        if isinstance(v, (bool, int, float, str, type(None))):
            return v
        if isinstance(v, (list, tuple)):
            return tuple(sig(x) for x in v)
        return type(v).__name__

    def wrap(name):
        orig = getattr(ops, name)

        def f(*a, **kw):
            calls.append((name, tuple(sig(v) for v in a), tuple(sorted((k, sig(v)) for k, v in kw.items()))))
            return orig(*a, **kw)
        monkeypatch.setattr(ops, name, f)
    for name in _TRACED:
        wrap(name)
    return calls


def _saved_forward(E, img, noises):
    from dge_amd.autograd_encpg import pg_encoder_forward
    _, z, saved = pg_encoder_forward(E, img, noises, save=True)
    return saved, R.randn("ep.gz", tuple(z.shape), 64).cuda()


def _backward_as_before(E, saved, g_z):
    """What pg_encoder_backward(E, saved, g_z) issued before it learnt need_img / params: the same ops, in that order."""
    from dge_amd import ops
    from dge_amd.enc_steps import blocks, conv_bwd, fromrgb_param_grads, grads_in_order, linear_backward, red_param_grads
    from dge_amd.weight_cache import pack_cache
    cache = pack_cache(E)
    dev = g_z.device
    B = g_z.shape[0]
    Rr = saved["img"].shape[2]
    dt = ops.dtype_of(saved["x0"])
    grads = {}
    g_flat = linear_backward(E.new_final, g_z.float().contiguous(), saved["flat"], grads, "new_final")
    L = len(saved["blocks"])
    C_last = E.decode_block[L - 1].inputs
    g_out = ops.nchw_to_nhwc(g_flat.view(B, C_last, Rr >> (L - 1), Rr >> (L - 1)), B, dt)
    for j, blk, rec, pre, Cc, C2, H, N in blocks(E, Rr, saved):
        x, x1 = rec["x"], rec["x1"]
        red1 = ops.zeros((Cc, 2), dev)
        if blk.has_second_conv:
            has3 = Cc != C2
            red2 = ops.zeros((C2, 2), dev)
            g_s = ops.act_bwd(g_out, rec["a"], rec["n2"], pool=True, scale=0.25, red=red2)
            red_param_grads(grads, pre, 2, red2)
            g_y2, dots2 = conv_bwd(cache, grads, pre + "conv_2", blk.conv_2, g_s, x1, dt, H, rec["sc2"], rec["sh2"])
            coef2 = ops.in_bwd_coef(dots2, None, rec["musig2"], rec["sc2"], rec["sh2"], N)
            g_pre1 = ops.in_bwd(g_y2, x1, coef2, noise=rec["n1"], act=True, red=red1)
            if has3:
                gam, bta = blk.instance_norm_3.weight.detach(), blk.instance_norm_3.bias.detach()
                style = torch.cat([gam - 1.0, bta]).unsqueeze(0).expand(B, -1).contiguous()
                coef3, gstyle = ops.sg1_in_bwd_coef(ops.dot_stats(g_s, rec["r3"]), rec["sc3"], rec["sh3"], style, N)
                gsum = ops._sum_over_batch(gstyle)
                grads[pre + "instance_norm_3.weight"], grads[pre + "instance_norm_3.bias"] = gsum[:C2], gsum[C2:]
                g_r3 = ops.in_bwd(g_s, rec["r3"], coef3)
                grads[pre + "conv_3.bias"] = ops.chan_sum(g_r3)
                extra, _ = conv_bwd(cache, grads, pre + "conv_3", blk.conv_3, g_r3, x, dt, None, dots=False)
            else:
                extra = g_s
        else:
            g_pre1 = ops.act_bwd(g_out, x1, rec["n1"], pool=False, scale=1.0, red=red1)
            extra = None
        red_param_grads(grads, pre, 1, red1)
        g_y1, dots1 = conv_bwd(cache, grads, pre + "conv_1", blk.conv_1, g_pre1, x, dt, H, rec["sc1"], rec["sh1"])
        coef1 = ops.in_bwd_coef(dots1, None, rec["musig1"], rec["sc1"], rec["sh1"], N)
        g_out = ops.in_bwd(g_y1, x, coef1, extra=extra, extra_pool=False, extra_scale=1.0)
    fromrgb_param_grads(E, saved, g_out, grads)
    return grads_in_order(E, grads)


@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_default_backward_issues_the_launches_it_issued_before(cd, monkeypatch):
    """Detached image, trained encoder (what e_align --mtype 3 runs): the traced op sequence and the KERNEL_LOG sequence of
    pg_encoder_backward equal those of the restatement above, and so do the gradients (deterministic mode: to the bit)."""
    from dge_amd import ops
    from dge_amd.autograd_encpg import pg_encoder_backward
    g = golden("encpg_imggrad.npz")
    E = _model(cd, g)
    img, noises = _inputs()
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        with torch.no_grad():
            saved, g_z = _saved_forward(E, img, noises)
            calls = _trace(monkeypatch)
            runs = []
            for fn in (pg_encoder_backward, _backward_as_before):
                del calls[:]
                ops.KERNEL_LOG = log = []
                try:
                    out = fn(E, saved, g_z)
                finally:
                    ops.KERNEL_LOG = None
                torch.cuda.synchronize()
                runs.append((list(calls), [n for n, _ in log], out))
    finally:
        ops.set_deterministic(was)
    (calls_a, log_a, out_a), (calls_b, log_b, out_b) = runs
    assert len(calls_a) > 40 and calls_a == calls_b
    assert log_a == log_b
    assert "in_bwd_fromrgb_img" not in [c[0] for c in calls_a] and "fromrgb_bwd" in [c[0] for c in calls_a]
    assert len(out_a) == len(out_b) and sum(x is not None for x in out_a) > 40
    for ga, gb in zip(out_a, out_b):
        assert (ga is None) == (gb is None)
        if ga is not None:
            assert torch.equal(ga, gb)


@pytest.mark.parametrize("cd", ["f32", "bf16"])
def test_frozen_backward_launches_no_parameter_gradient_and_keeps_the_bits(cd, monkeypatch):
    """params=False: no weight-gradient, bias / noise-weight reduction, instance_norm_3 sum, conv_3 bias sum, FromRGB-reduction or
    head-weight-gradient launch, every parameter gradient None, and g_img equal to the trained form's to the bit (deterministic
    mode).  The autograd function takes this form for an encoder whose parameters are frozen."""
    from dge_amd import ops
    from dge_amd.autograd_encpg import pg_encoder_backward
    g = golden("encpg_imggrad.npz")
    E = _model(cd, g)
    img, noises = _inputs()
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        with torch.no_grad():
            saved, g_z = _saved_forward(E, img, noises)
            grads_t, g_img_t = pg_encoder_backward(E, saved, g_z, need_img=True)
            calls = _trace(monkeypatch)
            ops.KERNEL_LOG = log = []
            try:
                grads_f, g_img_f = pg_encoder_backward(E, saved, g_z, need_img=True, params=False)
            finally:
                ops.KERNEL_LOG = None
            torch.cuda.synchronize()
        names = [n for n, _ in log]
        opsrun = [c[0] for c in calls]
        for bad in ("conv_wgrad", "dense_wgrad", "fromrgb_bwd", "chan_sum", "_sum_over_batch"):
            assert bad not in opsrun, (bad, opsrun)
        for c in calls:          # no reduction buffer goes into an activation / instance-norm backward
            if c[0] in ("act_bwd", "in_bwd"):
                assert dict(c[2]).get("red") is None, c
        for n in names:
            assert "wgrad" not in n and "fromrgb_bwd" not in n and not n.endswith(",fr>"), n
        tag = "bf16" if cd == "bf16" else "f32"
        assert names.count(f"in_bwd_fromrgb_img<{tag},data>") == 1, names
        assert all(x is None for x in grads_f) and any(x is not None for x in grads_t)
        assert g_img_f.shape == (2, 3, 64, 64) and torch.equal(g_img_f, g_img_t)
        # through autograd: frozen parameters select the same form
        monkeypatch.undo()
        for p in E.parameters():
            p.requires_grad_(False)
        x = img.clone().requires_grad_(True)
        _, z = E(x, noises=noises)
        z.backward(g_z)
        assert all(p.grad is None for p in E.parameters())
        assert torch.equal(x.grad, g_img_t)
    finally:
        ops.set_deterministic(was)


def test_unsupported_channel_count_takes_the_composed_passes(monkeypatch):
    """Where the kernel refuses the channel count the backward falls back to in_bwd -> fromrgb_dgrad -> fromrgb_bwd, with the same
    result up to the rounding of the stored gradient (f32: summation order only)."""
    from dge_amd import autograd_encpg, ops
    g = golden("encpg_imggrad.npz")
    E = _model("f32", g)
    img, noises = _inputs()
    with torch.no_grad():
        saved, g_z = _saved_forward(E, img, noises)
        grads_a, g_img_a = autograd_encpg.pg_encoder_backward(E, saved, g_z, need_img=True)
        monkeypatch.setattr(ops, "in_bwd_fromrgb_img_supported", lambda Cc, dt: False)

        def boom(*a, **kw):
            raise AssertionError("fused launch used for a refused channel count")
        monkeypatch.setattr(ops, "in_bwd_fromrgb_img", boom)
        grads_b, g_img_b = autograd_encpg.pg_encoder_backward(E, saved, g_z, need_img=True)
    assert _l2rel(g_img_b, g_img_a.cpu().numpy()) < 1e-5
    for (n, _), a, b in zip(E.named_parameters(), grads_a, grads_b):
        if n.startswith("FromRGB"):
            assert _l2rel(b, a.cpu().numpy()) < 1e-5, n
