"""Hand-written backward of the encoder (reference model/E/E.py:50-85,122-136 differentiated).

In E_align the gradient enters only through the latent codes w (E_align_s2.py:203-221: neither phase uses the
encoder's const output in a loss that is back-propagated).  Weights are re-packed from the
*current* parameter values at backward time, so the second backward of a step sees the weights
already updated by LREQAdam together with the activations saved before the update - the
reference's behaviour.

The inversion loop (embedding_v2_styleGAN2.py) also back-propagates a loss on the const output and through the encoder's input
(E(imgs2) of a generated image), with the encoder trained or frozen: encoder_backward's g_const / need_img / params.  The default
call (none of them) issues the E_align launches unchanged.
"""
import os
from types import SimpleNamespace

import torch

from . import ops
from .enc_steps import blocks, conv_bwd, grads_in_order, heads_backward, red_param_grads, skip_bwd
from .weight_cache import pack_cache, packed

FUSE_IN_BWD = not os.environ.get("DGE_NO_FUSED_IN_BWD")
FUSE_IMG_GRAD = not os.environ.get("DGE_NO_FUSED_IMG_GRAD")      # 1: the composed passes (A/B runs, tools/bench_embed_v2.py)

# the forms of conv_1's data gradient: reduced to the FromRGB parameter gradients in its epilogue (block 0), the block input's
# gradient out of its epilogue (blocks 1, 2), or the data gradient and the instance-norm backward as separate passes
FROMRGB, BLOCK_INPUT, SEPARATE = "FromRGB reduction", "block input", "separate passes"


def _conv2_part(c, blk, rec, pre, Cc, C2, H, g_out, gms2):
    """conv_2's part of a block: the block's output gradient g_out (in the last block, which has no conv_2: the gradient of the
    const output, or None) -> g_pre1, the gradient in front of conv_1's noise / bias / activation, and the skip gradient (extra,
    extra_pool, extra_scale) that the block input's gradient takes in."""
    B, dev, dt, grads, params = c.B, c.dev, c.dt, c.grads, c.params
    x1 = rec["x1"]
    extra, extra_pool, extra_scale = None, False, 1.0
    g_pre2 = g_y2 = dots2 = None
    fuse2 = False
    if blk.has_last_conv:
        has3 = Cc != C2
        # planar reductions ([k, C]): every parameter gradient below is a contiguous view, no strided copies
        red2 = ops.zeros((3 if has3 else 2, C2), dev) if params else None     # third row: sum of g_out = conv_3.bias gradient / 0.889
        g_pre2 = ops.act_bwd_mask(g_out, rec["m2"], rec["n2"], scale=0.111 * 0.25, red=red2, planar=True, defer=c.later)
        sum_g = red_param_grads(grads, pre, 2, red2, planar=True) if params else None
        gW2 = ops.zeros(tuple(blk.conv_2.weight.shape), dev) if params else None
        dots2 = ops.SlotStats(B, Cc, dev)                 # slot copies are added by in_bwd_coef
        # High-resolution blocks: the two sums the instance-norm backward needs come out of the weight-gradient launch, so the data
        # gradient can apply that backward (and the activation backward of conv_1's tail) in its epilogue - the in_bwd pass over
        # g_y2 and x1 below disappears (measured at batch 8: 410 -> 239 us at 1024^2, 212 -> 121 us at 512^2)
        if params and FUSE_IN_BWD and ops.conv_in_bwd_supported(B, H, H, C2, Cc, dt):
            fuse2 = ops.conv_wgrad_dots(g_pre2, x1, gW2, rec["sc2"], rec["sh2"], blk.conv_2.weight, dots2)
        if fuse2:
            grads[pre + "conv_2.weight"] = gW2
        else:
            g_y2, _ = conv_bwd(c.cache, grads, pre + "conv_2", blk.conv_2, g_pre2, x1, dt, H, rec["sc2"], rec["sh2"], params, dots=dots2,
                               dw=gW2)
        if has3:
            extra = skip_bwd(c.cache, grads, pre, blk, g_out, rec["xp"], dt, sum_g, params, post=c.post)
            extra_pool, extra_scale = True, 0.25
        else:
            extra, extra_pool, extra_scale = g_out, True, 0.889 * 0.25
    elif g_out is not None:
        # the last block with a gradient on the const output: out = 0.111*IN2(x1) + 0.889*x
        if Cc != C2:
            raise ops.DgeError("E.BE: a gradient on the const output of a last block with a channel change (conv_3 on the unpooled "
                               "input) is not implemented; not reachable with maxf-clamped widths")
        g_y2 = ops.blend(g_out, alpha=0.111)
        dots2 = ops.dot_stats(g_y2, x1)
        extra, extra_pool, extra_scale = g_out, False, 0.889
    coef2 = (dots2, gms2, rec["musig2"], rec["sc2"], rec["sh2"], H * H)          # computed inside in_bwd (dge_in_bwd_fused)
    red1 = ops.zeros((2, Cc), dev) if params else None
    if fuse2:
        redp = ops.SlotStats(B, Cc, dev)
        g_pre1 = ops.conv2d(g_pre2, packed(c.cache, blk.conv_2, dt, ops.PACK_DGRAD, H), Cc, 3, dot_src=x1,
                            in_bwd=dict(coef=ops.in_bwd_coef(*coef2), noise=rec["n1"].reshape(B, H, H), red=redp))
        ops._sum_planar(redp.buf.view(-1, Cc, 2), red1, c.later)
    else:
        g_pre1 = ops.in_bwd(g_y2, x1, coef2, noise=rec["n1"], act=True, red=red1, planar=True, defer=c.later)
    if params:
        red_param_grads(grads, pre, 1, red1, planar=True)
    return g_pre1, extra, extra_pool, extra_scale


def _conv1_form(c, j, Cc, H, extra, extra_pool):
    """The form conv_1's data gradient may take at block j, by the support predicates alone: nothing is launched here."""
    if not FUSE_IN_BWD or not c.params:      # (the fused forms take the instance-norm sums from the weight-gradient launch)
        return SEPARATE
    if j == 0 and c.need_img:                # FROMRGB stores nothing: the image gradient needs g_y1
        return SEPARATE
    if j == 0:
        # Block 0: the gradient w.r.t. the FromRGB output has one reader, the FromRGB parameter gradients.  With the instance-norm sums
        # out of the weight-gradient launch, the data gradient of conv_1 reduces them in its epilogue and stores nothing (the
        # in_bwd_fromrgb pass over g_y1, x0 and the image disappears, and so does the store of g_y1)
        ok = c.saved.get("img4") is not None and ops.conv_in_bwd_fromrgb_supported(c.B, H, H, Cc, Cc, c.dt)
        return FROMRGB if ok else SEPARATE
    # Blocks 1, 2: the same for the block input (instance-norm backward + pooled skip gradient, no activation) - the data gradient
    # stores the block's input gradient itself
    ok = (extra is None or extra_pool) and ops.conv_in_bwd_x_supported(c.B, H, H, Cc, Cc, c.dt)
    return BLOCK_INPUT if ok else SEPARATE


def _img_grad_fused(c, Cc):
    """Routing of block 0's last stage when the image gradient is wanted: ops.in_bwd_fromrgb_img where its kernel takes the channel
    count, else the composed passes in_bwd -> fromrgb_dgrad (-> fromrgb_bwd)."""
    return FUSE_IMG_GRAD and ops.in_bwd_fromrgb_img_supported(Cc, c.dt)


def _conv1_part(c, j, blk, rec, pre, Cc, H, g_pre1, gms1, extra, extra_pool, extra_scale):
    """conv_1's part of a block: g_pre1 and the skip gradient -> (the block input's gradient, or None at block 0 where it is
    reduced without being stored; the FromRGB reductions [4, C] then, else None).  With c.need_img block 0 also leaves the image
    gradient in c.g_img where one launch covers it."""
    B, dev, dt, grads = c.B, c.dev, c.dt, c.grads
    x = rec["x"]
    gW1 = ops.zeros(tuple(blk.conv_1.weight.shape), dev) if c.params else None
    dots1 = ops.SlotStats(B, Cc, dev)
    form = _conv1_form(c, j, Cc, H, extra, extra_pool)
    if form != SEPARATE:
        # the weight gradient that also leaves the instance-norm sums; where its kernel does not cover the shape (or in
        # deterministic mode) nothing has run and the separate passes take over
        covered = ops.conv_wgrad_dots(g_pre1, x, gW1, rec["sc1"], rec["sh1"], blk.conv_1.weight, dots1)
        if covered:
            grads[pre + "conv_1.weight"] = gW1
        else:
            form = SEPARATE
    coef1 = (dots1, gms1, rec["musig1"], rec["sc1"], rec["sh1"], H * H)
    if form == FROMRGB:
        frh = ops.SlotStats(B, Cc, dev)
        ops.conv2d(g_pre1, packed(c.cache, blk.conv_1, dt, ops.PACK_DGRAD, H), Cc, 3, dot_src=x, out=x.new_empty((1, 1, 1, 1)),
                   in_bwd=dict(coef=ops.in_bwd_coef(*coef1), fr=frh, img4=c.saved["img4"], extra=extra if extra_pool else None,
                               extra_scale=extra_scale))
        return None, ops._sum_planar(frh.buf.view(-1, Cc, 4), torch.empty((4, Cc), dtype=torch.float32, device=dev), c.later)
    if form == BLOCK_INPUT:
        return ops.conv2d(g_pre1, packed(c.cache, blk.conv_1, dt, ops.PACK_DGRAD, H), Cc, 3, dot_src=x,
                          in_bwd=dict(coef=ops.in_bwd_coef(*coef1), extra=extra, extra_scale=extra_scale)), None
    g_y1, _ = conv_bwd(c.cache, grads, pre + "conv_1", blk.conv_1, g_pre1, x, dt, H, rec["sc1"], rec["sh1"], c.params, dots=dots1, dw=gW1)
    if j == 0 and c.need_img and _img_grad_fused(c, Cc):
        # x is the FromRGB output and the image carries a gradient: instance-norm backward, FromRGB data gradient and (trained
        # encoder) the FromRGB parameter gradients in one launch; the gradient w.r.t. x is neither stored nor rounded
        c.g_img, fr = ops.in_bwd_fromrgb_img(g_y1, x, coef1, c.E.FromRGB.from_rgb.weight.detach(), c.saved["img"].float() if c.params else None,
                                             extra=extra, extra_pool=extra_pool, extra_scale=extra_scale, defer=c.later)
        return None, fr
    if j == 0 and Cc <= 512 and c.params and not c.need_img:
        # x is the FromRGB output: its gradient has one reader, the FromRGB parameter gradients - reduced in the same launch
        return None, ops.in_bwd_fromrgb(g_y1, x, coef1, c.saved["img"].float(), extra=extra, extra_pool=extra_pool,
                                        extra_scale=extra_scale, defer=c.later)
    return ops.in_bwd(g_y1, x, coef1, extra=extra, extra_pool=extra_pool, extra_scale=extra_scale), None


def encoder_backward(E, saved, g_w, g_const=None, need_img=False, params=True):
    """-> (gradients for E.parameters() in registration order - None where the reference produces none, e.g. the last block's
    noise_weight_2 / bias_2 - and the image gradient [B,3,R,R] f32 or None).
    g_const: the gradient of the const output [B,C,4,4] (a loss on it: space_loss(const2, const3) of embedding_v2), None without.
    need_img: the input image carries a gradient.  Block 0's conv_1 then takes the separate passes up to its data gradient, and the
    last launch (ops.in_bwd_fromrgb_img) gives the image gradient.
    params=False (frozen encoder: the W+ inversion mode): the data gradient alone.  No weight-gradient launch runs (conv_wgrad,
    conv_wgrad_dots, dense_wgrad, fromrgb_bwd), the side reductions that only feed parameter gradients and the DDP hook are
    dropped, every block runs the separate passes, and every parameter gradient is None.
    The default call issues the launches of E_align's backward, in their order."""
    if saved is None:
        raise RuntimeError("encoder forward ran without saved activations")
    L = E.layer_count
    B, dev = saved["img"].shape[0], saved["img"].device
    if g_w is None:      # a loss on the const output only: the statistics gradients of the heads are zero
        g_w = torch.zeros((B, 2 * L, E.latent_size), dtype=torch.float32, device=dev)
    # later: per-channel parameter-gradient reductions, one grouped launch (two with the DDP hook); post: what reads a deferred
    # sum runs after the flush
    c = SimpleNamespace(E=E, saved=saved, cache=pack_cache(E), grads={}, B=B, dev=dev, dt=ops.dtype_of(saved["x0"]),
                        later=ops.DeferredSums(), post=[], need_img=bool(need_img), params=bool(params), g_img=None)
    grads = c.grads

    def flush_sums():
        c.later.flush()
        for f in c.post:
            f()
        c.post.clear()
    # every inver_mod head at once (their gradient g_w is complete before the backward starts): two launches instead of 4 per block.
    # Their parameter gradients join `grads` with their block: the early hook below sees the deep blocks' gradients only.
    # (A frozen encoder drops them: the one-column kernels have no data-gradient-only form.)
    hgrads = {}
    gms_slot = heads_backward(saved["heads"], g_w, saved["musig_all"], hgrads)
    g_out = fr = None
    if g_const is not None:
        g_out = ops.nchw_to_nhwc(g_const.float(), B, c.dt)
    for j, blk, rec, pre, Cc, C2, H, _ in blocks(E, saved["img"].shape[2], saved):
        if params:
            for name in (pre + "inver_mod2", pre + "inver_mod1"):
                grads[name + ".weight"], grads[name + ".bias"] = hgrads[name + ".weight"], hgrads[name + ".bias"]
        if blk.has_last_conv and g_out is None:
            raise RuntimeError("non-final encoder block without an output gradient")
        g_pre1, extra, extra_pool, extra_scale = _conv2_part(c, blk, rec, pre, Cc, C2, H, g_out, gms_slot(2 * j + 1))
        g_out, fr = _conv1_part(c, j, blk, rec, pre, Cc, H, g_pre1, gms_slot(2 * j), extra, extra_pool, extra_scale)
        if j == L // 2 and params:
            # data-parallel runs: the gradients of blocks L-1 .. L/2 (the 512-channel blocks: > 90 % of the parameter bytes) are
            # complete here, while the high-resolution blocks still to come take most of the backward's time
            hook = E.__dict__.get("_early_grad_hook")
            if hook is not None:
                flush_sums()
                hook(dict(grads))
    if need_img and c.g_img is None:       # the composed passes: g_out is the stored gradient w.r.t. the FromRGB output
        c.g_img = ops.fromrgb_dgrad(g_out, saved["x0"], E.FromRGB.from_rgb.weight.detach())
    if params and fr is None:
        fr = ops.fromrgb_bwd(g_out, saved["x0"], saved["img"].float(), planar=True, defer=c.later)
    flush_sums()
    if params:
        grads["FromRGB.from_rgb.weight"] = fr[:3].t().reshape(E.startf, 3, 1, 1)
        grads["FromRGB.from_rgb.bias"] = fr[3]
    return grads_in_order(E, grads), c.g_img
