"""E_PG.BE (reference model/E/E_PG.py:73-108,150-164) forward / hand-written backward pipelines over the HIP ops.

Per block: IN -> conv3x3 -> +noise -> +bias -> lrelu -> IN -> conv3x3 -> +noise -> +bias -> (+ affine-IN(conv1x1(residual)))
-> lrelu -> avg_pool2d; the last block stops after the first lrelu; head `new_final` on the NCHW-flattened activation
(the evident intent).  The gradient enters through the head output only.

Backward building blocks (all in libdge_hip.so): `act_bwd` (lrelu' + pooling adjoint + bias / noise-weight sums),
`conv_wgrad`, data-gradient convs whose epilogue yields the two per-(b,c) sums the instance-norm backward needs,
`in_bwd_coef` / `in_bwd` (instance-norm backward as one streaming affine pass) and, for the affine instance norm of
the residual branch, `sg1_in_bwd_coef` with (gamma - 1, beta) in the role of StyleGAN1's per-sample style: its style
gradients summed over the batch are the gamma / beta gradients.
"""
import torch

from . import ops
from .enc_steps import blocks, conv_bwd, conv_fwd, draw_noises, fromrgb_param_grads, grads_in_order, linear_backward, red_param_grads
from .stylegan2_generator import _dt
from .weight_cache import pack_cache, packed


def pg_encoder_forward(E, img, noises=None, save=False):
    dt = _dt(E.compute_dtype)
    dev = img.device
    B, _, R, _ = img.shape
    if noises is None:
        noises = draw_noises(E, B, R, dev)
    cache = pack_cache(E)
    zeros = lambda c: ops.zeros((B, c, 2), dev)
    fr = E.FromRGB.from_rgb
    stats = zeros(E.startf)
    x = ops.fromrgb(img.float(), fr.weight.detach(), fr.bias.detach(), dt, stats)
    saved = {"img": img, "x0": x, "blocks": []} if save else None
    ni = 0
    for j, blk, _, _, Cc, C2, H, N in blocks(E, R):
        musig1, sc1, sh1 = ops.stats_finalize(stats, N)
        st1 = zeros(Cc)
        n1 = noises[ni].reshape(B, H, H).contiguous(); ni += 1
        x1 = conv_fwd(cache, blk, 1, x, Cc, dt, H, sc1, sh1, n1, stats=st1)
        rec = dict(x=x, musig1=musig1, sc1=sc1, sh1=sh1, n1=n1, x1=x1) if save else None
        if not blk.has_second_conv:
            if save:
                saved["blocks"].append(rec)
            x = x1
            break
        musig2, sc2, sh2 = ops.stats_finalize(st1, N)
        n2 = noises[ni].reshape(B, H, H).contiguous(); ni += 1
        pre2 = conv_fwd(cache, blk, 2, x1, C2, dt, H, sc2, sh2, n2, act=ops.ACT_NONE)
        if Cc != C2:
            st3 = zeros(C2)
            r3 = ops.conv2d(x, packed(cache, blk.conv_3, dt, ops.PACK_FWD), C2, 1, bias=blk.conv_3.bias.detach(), stats=st3)
            _, sc3, sh3 = ops.stats_finalize(st3, N)
            g, bta = blk.instance_norm_3.weight.detach(), blk.instance_norm_3.bias.detach()
            s = ops.blend(r3, z=pre2, sc=(sc3 * g).contiguous(), sh=(sh3 * g + bta).contiguous(), alpha=1.0, beta=1.0)
        else:
            r3 = sc3 = sh3 = None
            s = ops.blend(x, z=pre2, alpha=1.0, beta=1.0)
        a = ops.blur_noise_act(s, None, None, None, blur=False)          # leaky_relu(x + residual)
        nstats = zeros(C2)
        xn = ops.blend(a, pool=True, stats=nstats)                       # avg_pool2d
        if save:
            rec.update(musig2=musig2, sc2=sc2, sh2=sh2, n2=n2, r3=r3, sc3=sc3, sh3=sh3, a=a)
            saved["blocks"].append(rec)
        x, stats = xn, nstats
    xo = ops.nhwc_to_nchw(x)
    z = None
    if E.pggan:
        flat = xo.reshape(B, -1)
        z = ops.linear(flat, E.new_final.weight.detach(), E.new_final.bias.detach())
        if save:
            saved["flat"] = flat
    return xo, z, saved


FUSE_IMG_GRAD = True          # block 0's last stage with an image gradient: one launch (False: the composed passes, for timing)


def pg_encoder_backward(E, saved, g_z, need_img=False, params=True):
    """-> the gradients for E.parameters() in registration order; with need_img the pair (those, g_img [B,3,R,R] f32).
    need_img: the input image carries a gradient (embedding_v2_pggan: E(imgs2) of a generated image).  Block 0's last stage - the
    instance-norm backward on the FromRGB output plus the residual branch's gradient `extra` at full resolution, FromRGB's leaky-relu
    and data gradient and (trained encoder) its parameter reductions - is then one ops.in_bwd_fromrgb_img launch, which computes
    the instance-norm coefficients itself; where it refuses the channel count: in_bwd -> fromrgb_dgrad (-> fromrgb_bwd).
    params=False (frozen encoder: the z inversion mode): the data gradient alone.  No weight gradient, bias / noise-weight
    reduction, instance_norm_3 gamma / beta sum, conv_3 bias sum, FromRGB reduction or head weight gradient is launched, and every
    parameter gradient is None.
    The default call issues the launches of e_align --mtype 3's backward, in their order."""
    if saved is None:
        raise RuntimeError("E_PG forward ran without saved activations")
    cache = pack_cache(E)
    dev = g_z.device
    B = g_z.shape[0]
    R = saved["img"].shape[2]
    dt = ops.dtype_of(saved["x0"])
    grads = {}
    g_flat = linear_backward(E.new_final, g_z.float().contiguous(), saved["flat"], grads, "new_final", params)     # head: z = flat @ W^T + b
    L = len(saved["blocks"])
    C_last = E.decode_block[L - 1].inputs
    g_out = ops.nchw_to_nhwc(g_flat.view(B, C_last, R >> (L - 1), R >> (L - 1)), B, dt)
    g_img = fr = None
    for j, blk, rec, pre, Cc, C2, H, N in blocks(E, R, saved):
        x, x1 = rec["x"], rec["x1"]
        red1 = ops.zeros((Cc, 2), dev) if params else None
        if blk.has_second_conv:
            has3 = Cc != C2
            # s = pre2 + res ; a = lrelu(s) ; out = avg_pool(a)
            red2 = ops.zeros((C2, 2), dev) if params else None
            g_s = ops.act_bwd(g_out, rec["a"], rec["n2"], pool=True, scale=0.25, red=red2)
            if params:
                red_param_grads(grads, pre, 2, red2)
            g_y2, dots2 = conv_bwd(cache, grads, pre + "conv_2", blk.conv_2, g_s, x1, dt, H, rec["sc2"], rec["sh2"], params)
            coef2 = ops.in_bwd_coef(dots2, None, rec["musig2"], rec["sc2"], rec["sh2"], N)
            g_pre1 = ops.in_bwd(g_y2, x1, coef2, noise=rec["n1"], act=True, red=red1)
            if has3:
                gam, bta = blk.instance_norm_3.weight.detach(), blk.instance_norm_3.bias.detach()
                style = torch.cat([gam - 1.0, bta]).unsqueeze(0).expand(B, -1).contiguous()
                coef3, gstyle = ops.sg1_in_bwd_coef(ops.dot_stats(g_s, rec["r3"]), rec["sc3"], rec["sh3"], style, N)
                if params:
                    gsum = ops._sum_over_batch(gstyle)
                    grads[pre + "instance_norm_3.weight"], grads[pre + "instance_norm_3.bias"] = gsum[:C2], gsum[C2:]
                g_r3 = ops.in_bwd(g_s, rec["r3"], coef3)
                if params:
                    grads[pre + "conv_3.bias"] = ops.chan_sum(g_r3)
                extra, _ = conv_bwd(cache, grads, pre + "conv_3", blk.conv_3, g_r3, x, dt, None, params=params, dots=False)
            else:
                extra = g_s
        else:
            g_pre1 = ops.act_bwd(g_out, x1, rec["n1"], pool=False, scale=1.0, red=red1)
            extra = None
        if params:
            red_param_grads(grads, pre, 1, red1)
        g_y1, dots1 = conv_bwd(cache, grads, pre + "conv_1", blk.conv_1, g_pre1, x, dt, H, rec["sc1"], rec["sh1"], params)
        if j == 0 and need_img and FUSE_IMG_GRAD and ops.in_bwd_fromrgb_img_supported(Cc, dt):
            # x is the FromRGB output and the image carries a gradient: the gradient w.r.t. x is neither stored nor rounded
            g_img, fr = ops.in_bwd_fromrgb_img(g_y1, x, (dots1, None, rec["musig1"], rec["sc1"], rec["sh1"], N),
                                               E.FromRGB.from_rgb.weight.detach(), saved["img"].float() if params else None,
                                               extra=extra, extra_pool=False, extra_scale=1.0)
            g_out = None
        else:
            coef1 = ops.in_bwd_coef(dots1, None, rec["musig1"], rec["sc1"], rec["sh1"], N)
            g_out = ops.in_bwd(g_y1, x, coef1, extra=extra, extra_pool=False, extra_scale=1.0)
    if need_img and g_img is None:         # the composed passes: g_out is the stored gradient w.r.t. the FromRGB output
        g_img = ops.fromrgb_dgrad(g_out, saved["x0"], E.FromRGB.from_rgb.weight.detach())
    if params:
        if fr is None:
            fromrgb_param_grads(E, saved, g_out, grads)
        else:
            grads["FromRGB.from_rgb.weight"] = fr[:3].t().reshape(E.startf, 3, 1, 1)
            grads["FromRGB.from_rgb.bias"] = fr[3]
    out = grads_in_order(E, grads)
    return (out, g_img) if need_img else out


class PGEncoderFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, E, img, noises, *params):
        need_params = any(ctx.needs_input_grad[3:])
        need_img = bool(ctx.needs_input_grad[1])
        _, z, saved = pg_encoder_forward(E, img.detach(), noises, save=need_params or need_img)
        ctx.E, ctx.saved_acts, ctx.need_img, ctx.need_params = E, saved, need_img, need_params
        return z

    @staticmethod
    def backward(ctx, g_z):
        out = pg_encoder_backward(ctx.E, ctx.saved_acts, g_z, need_img=ctx.need_img, params=ctx.need_params)
        grads, g_img = out if ctx.need_img else (out, None)
        if g_img is not None:
            g_img = g_img.to(ctx.saved_acts["img"].dtype)
        return (None, g_img, None) + tuple(grads)
