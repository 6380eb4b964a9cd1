"""E_Blur encoder (reference model/E/E_Blur.py:16-134) forward / backward pipelines over the HIP ops.

Unlike E.BE inside E_align, the inversion loop (embedding_img.py:86-127) back-propagates through BOTH encoder
outputs (latents w and the 4x4 `const`) and through the encoder's INPUT (the second call encodes a generated image
that carries a gradient), so this backward returns parameter gradients and the image gradient.

Block forward (not last): IN1 -> conv_1 +noise+bias -> lrelu (x1) -> IN2 -> blur (y2) ->
  fused_scale (block resolution label >= 128): conv_2 stride 2 with transform_kernel == avg_pool(conv3x3) (lreq.py:145-147),
      then +noise+bias -> lrelu at half resolution;
  else: conv3x3 +noise+bias -> lrelu -> avg_pool.
out = 0.111*x2 + 0.889*(conv_3)(avg_pool(x)).  Last block: out = 0.111*IN2(x1) + 0.889*x.
"""
import os

import torch

from . import ops
from .enc_steps import (blocks, conv_bwd, conv_fwd, draw_noises, fromrgb_param_grads, grads_in_order, head_list, heads_backward,
                        heads_forward, heads_table, linear_backward, red_param_grads, skip_bwd, slot_view)
from .stylegan2_generator import _dt
from .weight_cache import pack_cache, packed, version

_DIRECT_ACCUMULATE = os.environ.get("DGE_AUTOGRAD_ACCUMULATE") != "1"


def blur_noises(E, B, R, dev):
    """Noise tensors in the reference's draw order; fused-scale blocks draw the second one at half resolution."""
    noises = draw_noises(E, B, R, dev)
    ni = 0
    for j, blk in enumerate(E.decode_block):
        ni += 1
        if blk.has_last_conv:
            if blk.fused_scale:
                r = (R >> j) // 2
                noises[ni] = ops.randn((B, 1, r, r), dev)
            ni += 1
    return noises


def heads_rows_layout(E, B, dev):
    """The row-list table of the heads of an encoder that declares `w_rows` (E_Blur_W, E_Blur_W_2; enc_steps.heads_table), one per
    (batch size, device).  A head without rows (inver_mod1 of E_Blur_W_2) has no entry."""
    return heads_table(E, head_list(E, E.w_rows), B, dev, rows=True)


def blur_encoder_forward(E, img, noises=None, save=False):
    dt = _dt(E.compute_dtype)
    dev = img.device
    B, _, R, _ = img.shape
    noise, heads = getattr(E, "noise", True), getattr(E, "heads", True)       # E_Blur_Z (BlurBEZ): neither
    # E_Blur_W / E_Blur_W_2 (`w_rows`): no head feeds the trunk, so all of them run as ONE launch after the last block, from a flat
    # buffer of the blocks' (mean, std) vectors, and write their rows of w directly
    lay = heads_rows_layout(E, B, dev) if getattr(E, "w_rows", None) else None
    musig_all = torch.empty(lay["total_m"], dtype=torch.float32, device=dev) if lay else None
    ms_slot = lambda i: slot_view(lay, musig_all, i, B) if lay else None
    if lay:
        heads = False          # (the per-head launches below are BlurBE's)
    if noises is None and noise:
        noises = blur_noises(E, B, R, dev)
    cache = pack_cache(E)
    zeros = lambda c: ops.zeros((B, c, 2), dev)
    fr = E.FromRGB.from_rgb
    stats = zeros(E.startf)
    x = ops.fromrgb(img.float(), fr.weight.detach(), fr.bias.detach(), dt, stats)
    saved = {"img": img, "x0": x, "blocks": [], "heads": lay, "musig_all": musig_all} if save else None
    ws, ni = [], 0
    for j, blk, _, _, Cc, C2, H, N in blocks(E, R):
        last = not blk.has_last_conv
        has3 = Cc != C2
        musig1, sc1, sh1 = ops.stats_finalize(stats, N, musig_out=ms_slot(2 * j))
        w1 = ops.linear(musig1, blk.inver_mod1.weight.detach(), blk.inver_mod1.bias.detach()) if heads else None
        n1 = None
        if noise:
            n1 = noises[ni].reshape(B, H, H).contiguous(); ni += 1
        st1 = zeros(Cc)
        x1 = conv_fwd(cache, blk, 1, x, Cc, dt, H, sc1, sh1, n1, stats=st1)
        musig2, sc2, sh2 = ops.stats_finalize(st1, N, musig_out=ms_slot(2 * j + 1))
        w2 = ops.linear(musig2, blk.inver_mod2.weight.detach(), blk.inver_mod2.bias.detach()) if heads else None
        rec = dict(x=x, musig1=musig1, sc1=sc1, sh1=sh1, n1=n1, x1=x1, musig2=musig2, sc2=sc2, sh2=sh2) if save else None
        nstats = zeros(C2) if not last else None
        if not last:
            y2 = ops.blur_noise_act(ops.blend(x1, sc=sc2, sh=sh2), None, None, None, blur=True, act=False)   # blur(IN2(x1))
            n2 = None
            if noise:
                r2 = H // 2 if blk.fused_scale else H
                n2 = noises[ni].reshape(B, r2, r2).contiguous(); ni += 1
            if blk.fused_scale:        # conv(s2, transform_kernel) == pool(conv); noise/bias/lrelu at half resolution
                t = ops.blend(ops.conv2d(y2, packed(cache, blk.conv_2, dt, ops.PACK_FWD, H), C2, 3), pool=True)
                a2 = x2 = ops.blur_noise_act(t, n2, blk.noise_weight_2.detach().reshape(-1) if noise else None,
                                             blk.bias_2.detach().reshape(-1), blur=False)
            else:
                a2 = conv_fwd(cache, blk, 2, y2, C2, dt, H, noise=n2)
                x2 = ops.blend(a2, pool=True)
            xp = ops.blend(x, pool=True)
            if has3:
                out = ops.conv2d(xp, packed(cache, blk.conv_3, dt, ops.PACK_FWD), C2, 1, bias=blk.conv_3.bias.detach(),
                                 gain=0.889, addend=x2, add_scale=0.111, stats=nstats)
            else:
                out = ops.blend(x2, z=xp, alpha=0.111, beta=0.889, stats=nstats)
            if save:
                rec.update(y2=y2, n2=n2, a2=a2, xp=xp if has3 else None)
                if blk.fused_scale and E.__dict__.get("_conv2_dgrad_at_forward"):
                    # the reference's strided conv_2 convolves with a tensor DERIVED from the weight at forward time
                    # (transform_kernel, model/utils/lreq.py:145-147), which autograd saves: its data gradient keeps reading the
                    # forward's values after an optimizer step, while every other layer (implicit lreq) reads the live parameter
                    rec["w2_fwd"] = (version(blk.conv_2.weight), blk.conv_2.weight.detach().clone())
        else:
            if has3:
                raise NotImplementedError("E_Blur: last block with a channel change is not reachable with maxf-clamped widths")
            out = ops.blend(x1, z=x, sc=sc2, sh=sh2, alpha=0.111, beta=0.889)
        if save:
            saved["blocks"].append(rec)
        ws = [w2, w1] + ws
        x, stats = out, nstats
    if lay:
        w = heads_forward(lay, musig_all, torch.empty((B, 2 * E.layer_count, lay["O"]), dtype=torch.float32, device=dev))
        return ops.nhwc_to_nchw(x), w, saved
    return ops.nhwc_to_nchw(x), (torch.stack(ws, dim=1) if heads else None), saved


def blur_encoder_backward(E, saved, g_w, g_const=None, need_img=False, params=True):
    """-> (gradients for E.parameters() in registration order, image gradient [B,3,R,R] or None).
    params=False (frozen encoder: the W+ inversion mode of embedding_v2.py): the data gradient alone.  No weight-gradient
    launch runs (conv_wgrad, the dense weight gradients, fromrgb_bwd) and the side reductions that only feed parameter
    gradients are dropped; the data path is the same launches in the same order, so the image gradient is the same bits.
    Every parameter gradient is None.
    An encoder without heads (E.heads False, E_Blur_Z) takes g_w=None: the statistics gradient fed to in_bwd_coef is then zero.
    Without noise (E.noise False) no noise-weight gradient is formed.
    An encoder with `w_rows` (E_Blur_W, E_Blur_W_2): g_w [B, 2L, O] with unit inner stride (row strides free); the backward of every
    head runs once, in front of the block loop (ops.heads_rows_bwd).  A head that feeds no row of w (inver_mod1 of E_Blur_W_2) gets
    no statistics gradient and None - not zeros - for its weight and bias."""
    cache = pack_cache(E)
    noise, heads = getattr(E, "noise", True), getattr(E, "heads", True)
    B, _, R, _ = saved["img"].shape
    dev = saved["img"].device
    L = E.layer_count
    grads = {}
    dt = ops.dtype_of(saved["x0"])
    g_out = None
    if g_const is not None:
        g_out = ops.nchw_to_nhwc(g_const.float().contiguous(), B, dt) if g_const.shape[0] == B else None
    gms_slot = heads_backward(saved["heads"], g_w, saved["musig_all"], grads, params) if saved["heads"] else None
    for j, blk, rec, pre, Cc, C2, H, N in blocks(E, R, saved):
        last = not blk.has_last_conv
        has3 = Cc != C2
        if gms_slot:
            gms2, gms1 = gms_slot(2 * j + 1), gms_slot(2 * j)
        elif not heads:
            gms2 = gms1 = None
        else:
            g_w2, g_w1 = g_w[:, 2 * (L - 1 - j)], g_w[:, 2 * (L - 1 - j) + 1]
            gms2 = linear_backward(blk.inver_mod2, g_w2, rec["musig2"], grads, pre + "inver_mod2", params)
            gms1 = linear_backward(blk.inver_mod1, g_w1, rec["musig1"], grads, pre + "inver_mod1", params)
        x, x1 = rec["x"], rec["x1"]
        extra, extra_pool, extra_scale = None, False, 1.0
        if not last:
            if g_out is None:
                raise RuntimeError("non-final encoder block without an output gradient")
            red2 = ops.zeros((C2, 3 if has3 else 2), dev) if params else None   # {bias_2, noise_weight_2 [, sum g_out -> conv_3.bias]}
            if blk.fused_scale:
                g_t = ops.act_bwd(g_out, rec["a2"], rec["n2"], pool=False, scale=0.111, red=red2)      # lrelu' at half resolution
                g_c2 = ops.nearest_up2(g_t, 0.25)                                                  # adjoint of the 2x2 average
            else:
                g_c2 = ops.act_bwd(g_out, rec["a2"], rec["n2"], pool=True, scale=0.111 * 0.25, red=red2)
            sum_g = None
            if params:
                sum_g = red_param_grads(grads, pre, 2, red2, noise=noise)
                gW2 = ops.zeros(tuple(blk.conv_2.weight.shape), dev)
                ops.conv_wgrad(g_c2, rec["y2"], gW2)
                grads[pre + "conv_2.weight"] = gW2
            snap = rec.get("w2_fwd")
            if snap is not None and snap[0] != version(blk.conv_2.weight):      # written since the forward: the forward's values
                w2pk = ops.pack_conv_weight(snap[1], ops.pack_mode_for(snap[1], ops.PACK_DGRAD, H, H, dt), dt, 1.0)
            else:
                w2pk = packed(cache, blk.conv_2, dt, ops.PACK_DGRAD, H)
            g_y2b = ops.conv2d(g_c2, w2pk, Cc, 3)
            g_y2 = ops.blur_noise_act(g_y2b, None, None, None, blur=True, act=False)                 # Blur is self-adjoint
            dots2 = ops.dot_stats(g_y2, x1)
            if has3:
                extra = skip_bwd(cache, grads, pre, blk, g_out, rec["xp"], dt, sum_g, params)
                extra_pool, extra_scale = True, 0.25
            else:
                extra, extra_pool, extra_scale = g_out, True, 0.889 * 0.25
        else:
            if g_out is not None:            # out = 0.111*IN2(x1) + 0.889*x
                g_y2 = ops.blend(g_out, alpha=0.111)
                dots2 = ops.dot_stats(g_y2, x1)
                extra, extra_pool, extra_scale = g_out, False, 0.889
            else:
                g_y2, dots2 = None, None
        coef2 = ops.in_bwd_coef(dots2, gms2, rec["musig2"], rec["sc2"], rec["sh2"], N)
        red1 = ops.zeros((Cc, 2), dev) if params else None
        g_pre1 = ops.in_bwd(g_y2, x1, coef2, noise=rec["n1"], act=True, red=red1)
        if params:
            red_param_grads(grads, pre, 1, red1, noise=noise)
        g_y1, dots1 = conv_bwd(cache, grads, pre + "conv_1", blk.conv_1, g_pre1, x, dt, H, rec["sc1"], rec["sh1"], params)
        coef1 = ops.in_bwd_coef(dots1, gms1, rec["musig1"], rec["sc1"], rec["sh1"], N)
        g_out = ops.in_bwd(g_y1, x, coef1, extra=extra, extra_pool=extra_pool, extra_scale=extra_scale)
    if params:
        fromrgb_param_grads(E, saved, g_out, grads)
    g_img = ops.fromrgb_dgrad(g_out, saved["x0"], E.FromRGB.from_rgb.weight.detach()) if need_img else None
    return grads_in_order(E, grads), g_img


class BlurEncoderFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, E, img, noises, *params):
        need = any(ctx.needs_input_grad[1:])
        xo, w, saved = blur_encoder_forward(E, img.detach(), noises, save=need)
        ctx.E, ctx.saved_acts = E, saved
        ctx.need_img = ctx.needs_input_grad[1]
        return xo, w

    @staticmethod
    def backward(ctx, g_x, g_w):
        if ctx.saved_acts is None:
            raise RuntimeError("E_Blur forward ran without saved activations")
        B = ctx.saved_acts["img"].shape[0]
        if g_w is None:
            g_w = torch.zeros((B, 2 * ctx.E.layer_count, ctx.E.latent_size), dtype=torch.float32, device=ctx.saved_acts["img"].device)
        frozen = not any(ctx.needs_input_grad[3:])      # no encoder parameter requires a gradient: data gradient only
        g_w = g_w.float()
        if not (getattr(ctx.E, "w_rows", None) and g_w.stride(2) == 1):      # (the grouped head backward reads strided rows)
            g_w = g_w.contiguous()
        grads, g_img = blur_encoder_backward(ctx.E, ctx.saved_acts, g_w, g_x, need_img=ctx.need_img, params=not frozen)
        return (None, g_img, None) + _param_grads_out(ctx.E, grads, frozen)


def _out_z_window(E, xo):
    """out_z = Conv2d(512, 512, 3, stride 2, padding 0) on the [B, 512, 4, 4] trunk output (E_Blur_Z.py:102,137) reads the top-left
    3x3 window only and produces one pixel: a dense layer over that window, flattened (c, kh, kw) as the weight is."""
    B, Cc, H, W = xo.shape
    if H != 4 or W != 4:
        raise ValueError(f"E_Blur_Z: out_z maps a 4x4 trunk output to 1x1; this encoder/input size gives {H}x{W}")
    return xo[:, :, :3, :3].contiguous().view(B, Cc * 9)


class BlurZEncoderFunction(torch.autograd.Function):
    """E_Blur_Z.BE: the E_Blur trunk without noise and heads (blur_encoder_forward / _backward) -> out_z -> z [B, 512, 1, 1].
    out_z runs on the existing dense kernels over the gathered 3x3 window (dge_linear forward, dge_linear_t data gradient,
    dge_dense_wgrad weight / bias gradient): at 1x1 output the convolution is exactly that matrix product, [B, 4608] x [4608, 512],
    and B <= 8 rows give a conv kernel nothing to tile.  Rows / columns 3 of the trunk output get zero gradient, as in the
    reference.  The backward reads out_z's weight as it is then (the reference's second backward runs on weights the first
    optimizer step already changed)."""

    @staticmethod
    def forward(ctx, E, img, *params):
        need = any(ctx.needs_input_grad[1:])
        xo, _, saved = blur_encoder_forward(E, img.detach(), None, save=need)
        win = _out_z_window(E, xo)
        oz = E.out_z
        z = ops.linear(win, oz.weight.detach().reshape(oz.weight.shape[0], -1), oz.bias.detach())
        ctx.E, ctx.saved_acts, ctx.win, ctx.C = E, saved, win, xo.shape[1]
        ctx.need_img = ctx.needs_input_grad[1]
        return z.view(z.shape[0], z.shape[1], 1, 1)

    @staticmethod
    def backward(ctx, g_z):
        if ctx.saved_acts is None:
            raise RuntimeError("E_Blur_Z forward ran without saved activations")
        E, win, Cc = ctx.E, ctx.win, ctx.C
        B = win.shape[0]
        oz = E.out_z
        Wz = oz.weight.detach().reshape(oz.weight.shape[0], -1)
        g = g_z.float().reshape(B, -1).contiguous()
        g_win = torch.empty_like(win)
        ops.linear_t(g, Wz, g_win)
        g_x = torch.zeros((B, Cc, 4, 4), dtype=torch.float32, device=g.device)
        g_x[:, :, :3, :3] = g_win.view(B, Cc, 3, 3)
        frozen = not any(ctx.needs_input_grad[2:])
        grads, g_img = blur_encoder_backward(E, ctx.saved_acts, None, g_x, need_img=ctx.need_img, params=not frozen)
        if not frozen:
            gW = torch.empty_like(oz.weight)
            gb = torch.empty_like(oz.bias)
            ops.dense_wgrad(g, win, gW.view(Wz.shape), gb)
            for k, (name, _) in enumerate(E.named_parameters()):
                if name == "out_z.weight":
                    grads[k] = gW
                elif name == "out_z.bias":
                    grads[k] = gb
        return (None, g_img) + _param_grads_out(E, grads, frozen)


def _param_grads_out(E, grads, frozen):
    """What a Function.backward of the family returns for the encoder's parameters: nothing for a frozen encoder, nothing when the
    gradients are added to `.grad` here (accumulate_param_grads, the default), else the gradients for autograd to accumulate."""
    if frozen or _DIRECT_ACCUMULATE:
        if not frozen:
            accumulate_param_grads(E, grads)
        return (None,) * len(grads)
    return tuple(grads)


def accumulate_param_grads(E, grads):
    """Adds the parameter gradients of ONE encoder call to `.grad` from inside the backward instead of handing them to autograd.
    The inversion loop (embedding_img.py:86-88) calls the encoder twice per iteration, so autograd's AccumulateGrad node clones every
    gradient of the first call (they are views of the step's zero-filled arena) and adds every gradient of the second: 2 x 105 launches
    of ~4 us per backward at batch 1, where the loop is paced by launches (profiles/r05_embed_kernel_stats.txt).  Here: one
    multi-tensor copy into a persistent flat buffer for the parameters without a gradient, one multi-tensor add for those with one.
    Same sums in the same order (first call, then second)."""
    params = list(E.parameters())
    lay = E.__dict__.get("_grad_flat")
    total = sum(p.numel() for p in params)
    if lay is None or lay["total"] != total or lay["buf"].device != params[0].device:
        buf = torch.zeros(total, dtype=torch.float32, device=params[0].device)
        views, o = [], 0
        for p in params:
            views.append(buf[o:o + p.numel()].view_as(p)); o += p.numel()
        lay = E.__dict__["_grad_flat"] = dict(total=total, buf=buf, views=views)
    first_dst, first_src, add_dst, add_src = [], [], [], []
    for p, v, g in zip(params, lay["views"], grads):
        if g is None:
            continue
        if p.grad is None:
            first_dst.append(v); first_src.append(g.reshape(p.shape))
            p.grad = v
        else:
            add_dst.append(p.grad); add_src.append(g.reshape(p.shape))
    if first_dst:
        torch._foreach_copy_(first_dst, first_src)
    if add_dst:
        torch._foreach_add_(add_dst, add_src)
