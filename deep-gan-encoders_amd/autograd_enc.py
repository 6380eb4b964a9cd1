"""Encoder forward / backward pipelines over the HIP ops, exposed as one autograd.Function
(PyTorch only routes the gradient tensors; every kernel is in libdge_hip.so)."""
import torch

from . import autograd_enc_bwd, ops
from .enc_steps import BE_W_ROWS, blocks, conv_fwd, draw_noises, head_list, heads_forward, heads_table, slot_view
from .stylegan2_generator import _dt
from .weight_cache import pack_cache, packed


def heads_layout(E, B, dev):
    """The one-column table of E.BE's heads (enc_steps.heads_table), one per (batch size, device)."""
    return heads_table(E, head_list(E, BE_W_ROWS), B, dev, rows=False)


def encoder_forward(E, img, noises=None, save=False, want_img4=True):
    """BE.forward (reference model/E/E.py:122-136) + BEBlock.forward (:50-85).  want_img4=False: the pixel-major image copy for the
    backward's FromRGB reduction is not emitted (a backward that wants the image gradient, or none for the parameters, never reads it)."""
    dt = _dt(E.compute_dtype)
    dev = img.device
    B, _, R, _ = img.shape
    if noises is None:
        noises = draw_noises(E, B, R, dev)
    cache = pack_cache(E)
    zeros = lambda c: ops.SlotStats(B, c, dev)        # statistics slots are added by stats_finalize itself
    fr = E.FromRGB.from_rgb
    stats = zeros(E.startf)
    # (training: the image also leaves in pixel-major form - the last data gradient of the backward reduces the FromRGB parameter
    #  gradients against it, autograd_enc_bwd.py)
    want4 = save and want_img4 and E.startf == 16 and not ops.is_deterministic() and ops.conv_in_bwd_fromrgb_supported(B, R, R, 16, 16, dt)
    x = ops.fromrgb(img.float(), fr.weight.detach(), fr.bias.detach(), dt, stats.plain(), img4=want4)
    img4 = None
    if want4:
        x, img4 = x
    lay = heads_layout(E, B, dev)
    musig_all = torch.empty(lay["total_m"], dtype=torch.float32, device=dev)     # all (mean, std) vectors, flat: grouped backward
    saved = {"img": img, "x0": x, "blocks": [], "img4": img4, "heads": lay, "musig_all": musig_all} if save else None
    ni = 0
    for j, blk, _, _, Cc, C2, H, N in blocks(E, R):
        last = not blk.has_last_conv
        musig1, sc1, sh1 = ops.stats_finalize(stats, N, musig_out=slot_view(lay, musig_all, 2 * j, B))
        n1 = noises[ni].reshape(B, H, H).contiguous(); ni += 1
        st1 = zeros(Cc)
        x1 = conv_fwd(cache, blk, 1, x, Cc, dt, H, sc1, sh1, n1, stats=st1)
        musig2, sc2, sh2 = ops.stats_finalize(st1, N, musig_out=slot_view(lay, musig_all, 2 * j + 1, B))
        rec = dict(x=x, musig1=musig1, sc1=sc1, sh1=sh1, n1=n1, x1=x1, musig2=musig2, sc2=sc2, sh2=sh2) if save else None
        has3 = Cc != C2
        nstats = zeros(C2) if not last else None
        if not last:
            n2 = noises[ni].reshape(B, H, H).contiguous(); ni += 1
            c2args = dict(in_scale=sc2, in_shift=sh2, noise=n2, noise_w=blk.noise_weight_2.detach().reshape(-1),
                          bias=blk.bias_2.detach().reshape(-1), act=ops.ACT_LRELU)
            m2 = None
            # the first blocks: conv_2 stores the 2x2 average pool of its result (and the signs for the backward) itself - the
            # full-resolution activation (537 MB at block 0) is neither written nor read back by a pooling pass
            pooled = has3 and ops.conv_pool_supported(B, H, H, Cc, C2, 3, dt)
            if pooled:
                r2 = ops.conv2d(x1, packed(cache, blk.conv_2, dt, ops.PACK_FWD, H), C2, 3, pool_out=True, pool_mask=save, **c2args)
                x2, m2 = r2 if save else (r2, None)
            else:
                a2 = ops.conv2d(x1, packed(cache, blk.conv_2, dt, ops.PACK_FWD, H), C2, 3, **c2args)
            if has3:
                if not pooled:
                    x2, m2 = ops.blend(a2, pool=True, mask=True) if save else (ops.blend(a2, pool=True), None)
                xp = ops.blend(x, pool=True)
                out = ops.conv2d(xp, packed(cache, blk.conv_3, dt, ops.PACK_FWD), C2, 1, bias=blk.conv_3.bias.detach(),
                                 gain=0.889, addend=x2, add_scale=0.111, stats=nstats)
            else:
                xp = ops.blend(x, pool=True, alpha=0.889)
                if save:
                    out, m2 = ops.blend(a2, z=xp, pool=True, alpha=0.111, beta=1.0, stats=nstats.plain(), mask=True)
                else:
                    out = ops.blend(a2, z=xp, pool=True, alpha=0.111, beta=1.0, stats=nstats.plain())
            if save:
                # a2 itself is not kept: its backward (lrelu derivative + pool adjoint) needs only the signs (1 bit per element)
                rec.update(n2=n2, m2=m2, xp=xp if has3 else None)
        else:
            if has3:
                y2 = ops.blend(x1, sc=sc2, sh=sh2)
                out = ops.conv2d(x, packed(cache, blk.conv_3, dt, ops.PACK_FWD), C2, 1, bias=blk.conv_3.bias.detach(),
                                 gain=0.889, addend=y2, add_scale=0.111)
            else:
                out = ops.blend(x1, z=x, sc=sc2, sh=sh2, alpha=0.111, beta=0.889)
        if save:
            saved["blocks"].append(rec)
        x, stats = out, nstats
    # every inver_mod head (w_l = musig_l @ W_l^T + b_l, E.py:51-53,64-66) in one launch: none of them feeds the trunk; column order
    # of w per E.py:130-134 (later / deeper blocks first) comes from the table
    w = heads_forward(lay, musig_all, torch.empty((B, 2 * E.layer_count, lay["O"]), dtype=torch.float32, device=dev))
    return ops.nhwc_to_nchw(x), w, saved


class EncoderFunction(torch.autograd.Function):
    """E.BE on the HIP path.  The backward takes gradients through both outputs (w and the const activation) and gives them to the
    parameters and, where it requires one, the input image (embedding_v2 back-propagates through E(imgs2) into the generator)."""

    @staticmethod
    def forward(ctx, E, img, noises, *params):
        need_img, need_params = ctx.needs_input_grad[1], any(ctx.needs_input_grad[3:])
        xo, w, saved = encoder_forward(E, img.detach(), noises, save=need_img or need_params, want_img4=need_params and not need_img)
        ctx.E, ctx.saved_acts = E, saved
        ctx.set_materialize_grads(False)      # an output that no loss uses arrives as None in backward
        return xo, w

    @staticmethod
    def backward(ctx, g_x, g_w):
        nparams = len(ctx.needs_input_grad[3:])
        if g_x is None and g_w is None:
            return (None, None, None) + (None,) * nparams
        frozen = not any(ctx.needs_input_grad[3:])      # no encoder parameter requires a gradient: data gradient only
        grads, g_img = autograd_enc_bwd.encoder_backward(ctx.E, ctx.saved_acts, g_w.float().contiguous() if g_w is not None else None,
                                                         g_x, need_img=ctx.needs_input_grad[1], params=not frozen)
        return (None, g_img, None) + (tuple(grads) if not frozen else (None,) * nparams)
