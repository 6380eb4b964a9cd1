"""space_loss (reference training_utils.py:54-99) and the three-scale image loss of
E_align_s2.py:185-203 on the HIP kernels, as autograd Functions whose forward also produces the
analytic gradient w.r.t. the second argument (the only one that carries grad in E_align).

image_loss_tsa_rows / space_loss_rows are the per-sample forms (embedding_v2 `independent`): sample b's loss is what image_loss_tsa
/ space_loss return on the one-row slices, the result is their sum over b (so the gradient of row b is the gradient of its own
loss) and the info tensors keep a row per sample."""
import contextlib
import os

import torch

from . import ops
from ._lib import lib, check
from .collectives import all_reduce
from .ops import _f32, _p, _stream


class GlobalBatch:
    """Makes the batch-coupled terms of space_loss (cosine over the batch-flattened vector, means,
    the 1/N of mse / ssim / lpips) refer to the GLOBAL batch of a data-parallel run: the per-rank
    partial sums are all-reduced before the loss and its gradient are formed."""

    def __init__(self, world):
        self.world = world

    def reduce(self, t):
        all_reduce(t)
        return t


def _pool_factor(h):
    k = 1
    while h > 256:          # training_utils.py:81 tests shape[2] only
        h //= 2
        k *= 2
    return k


def attention_windows(H, W):
    """(y0, x0, h, w) of the full image, AT1 and AT2 (E_align_s2.py:188-199)."""
    oy, ox = H // 8 + H // 32, W // 8 + W // 32
    return [(0, 0, H, W), (0, W // 8, H, W - 2 * (W // 8)), (oy, ox, H - 2 * oy, W - 2 * ox)]


_PK = 48          # floats per window in the packed reduction buffer: [0:8] the 8 sums, [8:40] SSIM slot copies, [40] LPIPS mean


def _window_reduce(a, b, win, image_space, lpips_model, need_grad, pk, world):
    """Pass 1 of one space_loss window: every per-rank partial sum goes into the packed row `pk` ([_PK] view, pre-zeroed), so
    that a data-parallel run exchanges ALL windows of a phase in one all-reduce.  Returns the state pass 2 needs."""
    B, Cc, H, W = a.shape
    y0, x0, h, w = win
    dev = a.device
    L = lib()
    slots = ops.zeros((16, 8), dev)         # 16 slot copies of the 8 sums (atomics contention), added up below
    check(L.dge_loss_reduce(_f32(a), _f32(b), _p(slots), B, Cc, H, W, y0, x0, h, w, _stream()), "dge_loss_reduce")
    ops._sum_over_batch(slots, pk[0:8])
    st = dict(win=win, pk=pk, k=1, npool=1.0, n=float(B * Cc * h * w) * world, lp=None, ap=None)
    if image_space:
        k = _pool_factor(h)
        hp, wp = h // k, w // k
        ap = torch.empty((B, Cc, hp, wp), dtype=torch.float32, device=dev)
        bp = torch.empty_like(ap)
        check(L.dge_crop_pool(_f32(a), _p(ap), B * Cc, H, W, y0, x0, h, w, k, _stream()), "dge_crop_pool")
        check(L.dge_crop_pool(_f32(b), _p(bp), B * Cc, H, W, y0, x0, h, w, k, _stream()), "dge_crop_pool")
        dmap = torch.empty((3, B, Cc, hp, wp), dtype=torch.float32, device=dev) if need_grad else None
        # pk[8:40]: 32 slot copies of the SSIM sum (atomics contention), added up by the finaliser
        check(L.dge_ssim_fwd(_p(ap), _p(bp), _p(pk[8:40]), _p(dmap), B * Cc, hp, wp, _stream()), "dge_ssim_fwd")
        st.update(k=k, npool=float(B * Cc * hp * wp) * world, ap=ap, bp=bp, dmap=dmap, g_lp=None)
        if lpips_model is not None:
            lp, st["g_lp"] = lpips_model.value_and_grad(ap, bp, need_grad=need_grad)       # mean over the rank's batch, d/dbp
            if world > 1:      # global mean = sum over ranks of (rank mean / world): joins the packed exchange
                check(L.dge_axpy_scalar(_p(lp), None, _p(pk[40:41]), 1, 1.0 / world, 0, _stream()), "dge_axpy_scalar")
                lp = pk[40:41]
            st["lp"] = lp
    return st


def _window_finish(a, b, st, image_space, weight, g_out, accumulate, world):
    """Pass 2: loss terms from the (globally reduced) sums and, when g_out is given, weight * dloss/db added into it."""
    B, Cc, H, W = a.shape
    y0, x0, h, w = st["win"]
    dev = a.device
    L = lib()
    pk = st["pk"]
    out8 = torch.empty(8, dtype=torch.float32, device=dev)
    gp = None
    if image_space and g_out is not None:
        bp = st["bp"]
        gp = torch.empty_like(bp)
        check(L.dge_ssim_bwd(_p(st["ap"]), _p(bp), _p(st["dmap"]), _p(gp), B * Cc, bp.shape[2], bp.shape[3], -1.0 / st["npool"], 0,
                             _stream()), "dge_ssim_bwd")
        if st["g_lp"] is not None:
            check(L.dge_axpy_scalar(_p(st["g_lp"]), None, _p(gp), gp.numel(), 2.0 / world, 1, _stream()), "dge_axpy_scalar")
    check(L.dge_space_loss_finalize(_p(pk[0:8]), _p(pk[8:40]) if image_space else None, _p(st["lp"]), _p(out8), st["n"], st["npool"],
                                    1 if image_space else 0, _stream()), "dge_space_loss_finalize")
    if g_out is not None:
        check(L.dge_space_loss_bwd(_f32(a), _f32(b), _p(pk[0:8]), _p(gp), _p(g_out), B * Cc, H, W, y0, x0, h, w, st["k"], st["n"],
                                   float(weight), 1 if accumulate else 0, _stream()), "dge_space_loss_bwd")
    return out8


def _space_loss_windows(a, b, wins, image_space, lpips_model, weights, g_outs, accumulate, gb=None):
    """space_loss on several windows of a, b [B,C,H,W] (training_utils.py:54-99 each): all reductions first, ONE exchange of the
    packed partial sums in a data-parallel run (`gb`), then the loss terms and gradients.  Returns the list of out8 tensors."""
    world = gb.world if gb is not None else 1
    pack = ops.zeros((len(wins), _PK), a.device)
    sts = [_window_reduce(a, b, win, image_space, lpips_model, g_outs[i] is not None, pack[i], world) for i, win in enumerate(wins)]
    if gb is not None:
        gb.reduce(pack)
    return [_window_finish(a, b, st, image_space, weights[i], g_outs[i], accumulate, world) for i, st in enumerate(sts)]


# DGE_SIDE_STREAMS=0: everything on the caller's stream (PMC counter collection serialises kernels; profiles of single stages)
_WINDOW_STREAMS = os.environ.get("DGE_WINDOW_STREAMS", "1") != "0" and os.environ.get("DGE_SIDE_STREAMS", "1") != "0"
_SIDE = {}


def _side_streams(dev, n):
    """n side streams of the device, created once (stream creation inside a step would be a host synchronisation)."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device())
    have = _SIDE.setdefault(key, [])
    while len(have) < n:
        have.append(torch.cuda.Stream(device=dev))
    return have[:n]


def _window_streams(dev, lpips_model, nw, npix):
    """(caller's stream, the side streams the windows 1.. of a merged-window loss fork to - none when they stay on one stream)"""
    main = torch.cuda.current_stream(dev) if dev.type == "cuda" else None
    # (the stream switches cost ~1 ms of host time per step: taken where the GPU work hides them - >= 4 Mpixel per call - or
    #  where the host is out of the picture, i.e. while a hipGraph is being captured)
    fork = (main is not None and lpips_model is not None and nw > 1 and _WINDOW_STREAMS and not ops.is_deterministic()
            and getattr(lpips_model, "_streams_warm", False)
            and (npix >= (4 << 20) or torch.cuda.is_current_stream_capturing()))
    return main, (_side_streams(dev, nw - 1) if fork else [])


def _space_loss_windows3(a, b, wins, lpips_model, weights, g, need, gb=None, g_split=None):
    """The three nested attention windows of image_loss_tsa with every image pass merged (dge_loss_reduce3, dge_crop_pool_multi,
    dge_space_loss_bwd3): `g` (or None) is WRITTEN with the weighted sum of the windows' gradients; need[i] False leaves window i
    out of the gradient.  Same arithmetic as _window_reduce / _window_finish per window.
    `g_split` (image_losses_split; `g` is None then): one full-size image or None per window, each WRITTEN with its own window's
    weighted gradient (dge_space_loss_bwd_split) instead of the sum."""
    import ctypes as C
    B, Cc, H, W = a.shape
    dev = a.device
    L = lib()
    world = gb.world if gb is not None else 1
    nw = len(wins)
    pack = ops.zeros((nw, _PK), dev)
    slots = ops.zeros((nw, 16, 8), dev)
    wflat = (C.c_int * (4 * nw))(*[int(v) for win in wins for v in win])
    check(L.dge_loss_reduce3(_f32(a), _f32(b), _p(slots), B, Cc, H, W, wflat, nw, _stream()), "dge_loss_reduce3")
    sums = ops.DeferredSums()
    for i in range(nw):
        sums.add(slots[i].view(16, 8, 1), pack[i, 0:8])      # [nslot, C = 8, NS = 1] -> the 8 sums of window i
    sums.flush()
    ks = [_pool_factor(win[2]) for win in wins]
    aps = [torch.empty((B, Cc, win[2] // k, win[3] // k), dtype=torch.float32, device=dev) for win, k in zip(wins, ks)]
    bps = [torch.empty_like(t) for t in aps]
    srcs = (C.c_void_p * (2 * nw))(*([a.data_ptr()] * nw + [b.data_ptr()] * nw))
    dsts = (C.c_void_p * (2 * nw))(*([t.data_ptr() for t in aps] + [t.data_ptr() for t in bps]))
    w2 = (C.c_int * (8 * nw))(*([int(v) for win in wins for v in win] * 2))
    k2 = (C.c_int * (2 * nw))(*(ks * 2))
    check(L.dge_crop_pool_multi(srcs, dsts, w2, k2, 2 * nw, B * Cc, H, W, _stream()), "dge_crop_pool_multi")
    sts = []
    # The windows are independent from here to the join below, and their LPIPS launches are small (conv3 - conv5 on 16^2 .. 64^2
    # features: 256 - 1152 workgroups, one or two per CU, each a serial weight stream): on one stream they run one after the
    # other on a half-empty chip.  Each window gets its own stream (forked off the caller's, joined before the results are
    # read); the first call stays on one stream (it fills the LPIPS weight-pack cache), so does the deterministic mode (its
    # slot workspace belongs to one stream at a time).
    main, side = _window_streams(dev, lpips_model, nw, B * H * W)
    fork = bool(side)
    for i, win in enumerate(wins):
        y0, x0, h, w = win
        ap, bp, k = aps[i], bps[i], ks[i]
        hp, wp = h // k, w // k
        ng = (g is not None or g_split is not None) and need[i]
        strm = side[i - 1] if (fork and i > 0) else None
        if strm is not None:
            strm.wait_stream(main)
        with (torch.cuda.stream(strm) if strm is not None else contextlib.nullcontext()):
            dmap = torch.empty((3, B, Cc, hp, wp), dtype=torch.float32, device=dev) if ng else None
            check(L.dge_ssim_fwd(_p(ap), _p(bp), _p(pack[i, 8:40]), _p(dmap), B * Cc, hp, wp, _stream()), "dge_ssim_fwd")
            st = dict(win=win, pk=pack[i], k=k, npool=float(B * Cc * hp * wp) * world, n=float(B * Cc * h * w) * world, ap=ap, bp=bp,
                      dmap=dmap, g_lp=None, lp=None, ng=ng)
            if lpips_model is not None:
                lp, st["g_lp"] = lpips_model.value_and_grad(ap, bp, need_grad=ng)
                if world > 1:
                    check(L.dge_axpy_scalar(_p(lp), None, _p(pack[i, 40:41]), 1, 1.0 / world, 0, _stream()), "dge_axpy_scalar")
                    lp = pack[i, 40:41]
                st["lp"] = lp
            # the window's pooled-image gradient (SSIM + LPIPS; neither needs the global sums) in the window's stream too
            st["gp"] = None
            if ng:
                gp = torch.empty_like(bp)
                check(L.dge_ssim_bwd(_p(ap), _p(bp), _p(dmap), _p(gp), B * Cc, hp, wp, -1.0 / st["npool"], 0, _stream()), "dge_ssim_bwd")
                if st["g_lp"] is not None:
                    check(L.dge_axpy_scalar(_p(st["g_lp"]), None, _p(gp), gp.numel(), 2.0 / world, 1, _stream()), "dge_axpy_scalar")
                st["gp"] = gp
        if strm is not None:            # results allocated on the side stream are read (and freed) under the caller's stream
            for t in (dmap, st["g_lp"], st["lp"], st["gp"]):
                if t is not None:
                    t.record_stream(main)
        sts.append(st)
    for strm in side:
        main.wait_stream(strm)
    if lpips_model is not None:
        lpips_model._streams_warm = True
    if gb is not None:
        gb.reduce(pack)
    outs, gps = [], []
    for i, st in enumerate(sts):
        gps.append(st["gp"])
        out8 = torch.empty(8, dtype=torch.float32, device=dev)
        check(L.dge_space_loss_finalize(_p(pack[i, 0:8]), _p(pack[i, 8:40]), _p(st["lp"]), _p(out8), st["n"], st["npool"], 1, _stream()),
              "dge_space_loss_finalize")
        outs.append(out8)
    if g is not None:
        sp = (C.c_void_p * nw)(*[pack[i, 0:8].data_ptr() for i in range(nw)])
        gpp = (C.c_void_p * nw)(*[(t.data_ptr() if t is not None else None) for t in gps])
        nn = (C.c_float * nw)(*[st["n"] for st in sts])
        ww = (C.c_float * nw)(*[float(weights[i]) if sts[i]["ng"] else 0.0 for i in range(nw)])
        kk = (C.c_int * nw)(*ks)
        check(L.dge_space_loss_bwd3(_f32(a), _f32(b), sp, gpp, _p(g), B * Cc, H, W, wflat, kk, nn, ww, nw, _stream()), "dge_space_loss_bwd3")
    if g_split is not None:
        _bwd_split(a, b, wins, [pack[i, 0:8] for i in range(nw)], gps, ks, [st["n"] for st in sts],
                   [float(weights[i]) if sts[i]["ng"] else 0.0 for i in range(nw)], g_split)
    return outs


def _bwd_split(a, b, wins, sums, gps, ks, ns, wts, outs):
    """One dge_space_loss_bwd_split launch: outs[k] (or None) is WRITTEN with wts[k] * (window k's gradient), zeros outside it."""
    import ctypes as C
    if all(t is None for t in outs):
        return
    B, Cc, H, W = a.shape
    nw = len(wins)
    ptrs = lambda ts: (C.c_void_p * nw)(*[(t.data_ptr() if t is not None else None) for t in ts])
    wflat = (C.c_int * (4 * nw))(*[int(v) for win in wins for v in win])
    check(lib().dge_space_loss_bwd_split(_f32(a), _f32(b), ptrs(sums), ptrs(gps), ptrs(outs), B * Cc, H, W, wflat, (C.c_int * nw)(*ks),
                                         (C.c_float * nw)(*ns), (C.c_float * nw)(*wts), nw, _stream()), "dge_space_loss_bwd_split")
    ops.log_kernel()


def _space_loss_windows_split(a, b, wins, lpips_model, weights, g_split, gb=None):
    """_space_loss_windows3 with g_split in deterministic mode: the per-window reductions of _window_reduce (dge_loss_reduce3 is
    not offered there), the pooled gradients of _window_finish, then the same single dge_space_loss_bwd_split launch."""
    B, Cc = a.shape[:2]
    L = lib()
    world = gb.world if gb is not None else 1
    pack = ops.zeros((len(wins), _PK), a.device)
    sts = [_window_reduce(a, b, win, True, lpips_model, g_split[i] is not None, pack[i], world) for i, win in enumerate(wins)]
    if gb is not None:
        gb.reduce(pack)
    outs, gps = [], []
    for i, st in enumerate(sts):
        gp = None
        if g_split[i] is not None:
            bp = st["bp"]
            gp = torch.empty_like(bp)
            check(L.dge_ssim_bwd(_p(st["ap"]), _p(bp), _p(st["dmap"]), _p(gp), B * Cc, bp.shape[2], bp.shape[3], -1.0 / st["npool"], 0,
                                 _stream()), "dge_ssim_bwd")
            if st["g_lp"] is not None:
                check(L.dge_axpy_scalar(_p(st["g_lp"]), None, _p(gp), gp.numel(), 2.0 / world, 1, _stream()), "dge_axpy_scalar")
        gps.append(gp)
        outs.append(_window_finish(a, b, st, True, weights[i], None, False, world))
    _bwd_split(a, b, wins, [pack[i, 0:8] for i in range(len(wins))], gps, [st["k"] for st in sts], [st["n"] for st in sts],
               [float(weights[i]) if g_split[i] is not None else 0.0 for i in range(len(wins))], g_split)
    return outs


def _space_loss_window(a, b, win, image_space, lpips_model, weight, g_out, accumulate, gb=None):
    return _space_loss_windows(a, b, [win], image_space, lpips_model, [weight], [g_out], accumulate, gb)[0]


class _ScaledGrad(torch.autograd.Function):
    """loss tensor whose gradient w.r.t. `b` was computed analytically in the forward."""

    @staticmethod
    def forward(ctx, b, loss, g):
        ctx.save_for_backward(g)
        return loss.clone()

    @staticmethod
    def backward(ctx, go):
        (g,) = ctx.saved_tensors
        out = torch.empty_like(g)
        check(lib().dge_axpy_scalar(_p(g), _p(go.contiguous().float()), _p(out), g.numel(), 1.0, 0, _stream()), "dge_axpy_scalar")
        return out, None, None


class _ScaledGrad2(torch.autograd.Function):
    """as _ScaledGrad, for a loss whose BOTH arguments carry a gradient (latent losses of embedding_img.py:118-124)."""

    @staticmethod
    def forward(ctx, a, b, loss, ga, gb):
        ctx.save_for_backward(ga, gb)
        return loss.clone()

    @staticmethod
    def backward(ctx, go):
        outs = []
        gof = go.contiguous().float()
        for g in ctx.saved_tensors:
            out = torch.empty_like(g)
            check(lib().dge_axpy_scalar(_p(g), _p(gof), _p(out), g.numel(), 1.0, 0, _stream()), "dge_axpy_scalar")
            outs.append(out)
        return outs[0], outs[1], None, None, None


def image_loss_tsa(imgs1, imgs2, lpips_model=None, weights=(1.0, 5.0, 9.0), global_batch=None, grad_windows=(True, True, True)):
    """loss_tsa = loss_imgs + 5*loss_medium + 9*loss_small (E_align_s2.py:185-203).
    Returns (loss [] on device, info [3,8] on device: rows full/AT1/AT2, columns
    loss, mse, mse_mean, mse_std, kl, cos, ssim, lpips).  No host synchronisation."""
    a = imgs1.detach().float().contiguous()
    b = imgs2.detach().float().contiguous()
    need = imgs2.requires_grad and torch.is_grad_enabled()
    wins = attention_windows(a.shape[2], a.shape[3])
    # grad_windows[i] False: the window enters the loss VALUE only (embedding_img.py:95-107 detaches both crops)
    if not ops.is_deterministic():       # every pass over the two images merged over the three windows
        g = torch.empty_like(b) if need else None
        infos = _space_loss_windows3(a, b, wins, lpips_model, weights, g, [bool(need and grad_windows[i]) for i in range(3)], gb=global_batch)
    else:
        g = torch.zeros_like(b) if need else None
        infos = _space_loss_windows(a, b, wins, True, lpips_model, weights,
                                    [g if (need and grad_windows[i]) else None for i in range(3)], accumulate=True, gb=global_batch)
    info = torch.stack(infos)
    loss = info[0, 0] * float(weights[0]) + info[1, 0] * float(weights[1]) + info[2, 0] * float(weights[2])   # no host->device copy
    if need:
        loss = _ScaledGrad.apply(imgs2, loss, g)
    return loss, info


def image_losses_split(imgs1, imgs2, lpips_model=None, weights=(1.0, 5.0, 9.0), windows=(True, True, True), global_batch=None):
    """The three image losses of the per-loss-update loop (ablation_utils/8.E_align_x_AT1_AT2.py:72-101), each with a gradient of
    its own: returns ([loss_imgs, 5*loss_medium, 9*loss_small], info [3,8] as image_loss_tsa).  One evaluation serves all three:
    the reductions, crops, SSIM and LPIPS passes are image_loss_tsa's, and one dge_space_loss_bwd_split launch writes the three
    gradient images.  windows[k] False: loss k is a plain value (its info row is kept), no gradient work is done for it.
    No host synchronisation."""
    a = imgs1.detach().float().contiguous()
    b = imgs2.detach().float().contiguous()
    need = imgs2.requires_grad and torch.is_grad_enabled()
    wins = attention_windows(a.shape[2], a.shape[3])
    want = [bool(need and windows[i]) for i in range(3)]
    gs = [torch.empty_like(b) if want[i] else None for i in range(3)]
    if not ops.is_deterministic():
        infos = _space_loss_windows3(a, b, wins, lpips_model, weights, None, want, gb=global_batch, g_split=gs)
    else:
        infos = _space_loss_windows_split(a, b, wins, lpips_model, weights, gs, gb=global_batch)
    info = torch.stack(infos)
    out = []
    for i in range(3):
        loss = info[i, 0] * float(weights[i])
        out.append(_ScaledGrad.apply(imgs2, loss, gs[i]) if want[i] else loss)
    return out, info


def space_loss(imgs1, imgs2, image_space=True, lpips_model=None, global_batch=None):
    """Drop-in for training_utils.space_loss; returns (loss tensor, info tensor[8] on device)
    instead of Python floats (the reference's 7 .item() syncs per call are deferred)."""
    a = imgs1.detach().float().contiguous()
    b = imgs2.detach().float().contiguous()
    need = imgs2.requires_grad and torch.is_grad_enabled()
    g = torch.empty_like(b) if need else None
    if image_space:
        B, Cc, H, W = a.shape
        out8 = _space_loss_window(a, b, (0, 0, H, W), True, lpips_model, 1.0, g, accumulate=False, gb=global_batch)
    else:
        # 3-D latents: the implicit softmax dim is 0 (the batch) -> planes = batch (training_utils.py:67)
        Bt = a.shape[0]
        n_in = a.numel() // Bt
        if a.dim() == 2:
            # 2-D latents (PGGAN / BigGAN z): the implicit softmax dim is 1 -> one softmax per sample over the features
            out8 = _space_loss_window(a.view(Bt, n_in, 1, 1), b.view(Bt, n_in, 1, 1), (0, 0, 1, 1), False, None, 1.0,
                                      g.view(Bt, n_in, 1, 1) if need else None, accumulate=False, gb=global_batch)
            loss = out8[0]
            return (_ScaledGrad.apply(imgs2, loss, g) if need else loss), out8
        out8 = _space_loss_window(a.view(1, Bt, 1, n_in), b.view(1, Bt, 1, n_in), (0, 0, 1, n_in), False, None, 1.0,
                                  g.view(1, Bt, 1, n_in) if need else None, accumulate=False, gb=global_batch)
        if imgs1.requires_grad and torch.is_grad_enabled():
            # the first argument carries a gradient too: 5*mse + 3*cos is symmetric, so d/da is the same kernel with
            # the arguments exchanged (the logged-only KL term is not, and is taken from the first evaluation)
            ga = torch.empty_like(a)
            _space_loss_window(b.view(1, Bt, 1, n_in), a.view(1, Bt, 1, n_in), (0, 0, 1, n_in), False, None, 1.0,
                               ga.view(1, Bt, 1, n_in), accumulate=False, gb=global_batch)
            gbt = g if need else torch.zeros_like(b)
            return _ScaledGrad2.apply(imgs1, imgs2, out8[0], ga, gbt), out8
    loss = out8[0]
    if need:
        loss = _ScaledGrad.apply(imgs2, loss, g)
    return loss, out8


# ------------------------------------------------------------------ per-sample forms
def _space_loss_rows(a, b, wins, image_space, lpips_model, weights, need, ga=None, gb=None):
    """space_loss of every sample of a, b [B,C,H,W] on up to 3 nested windows (all inside window 0), the samples kept apart:
    dge_loss_reduce_rows, dge_crop_pool_multi, per window dge_ssim_fwd_rows + per-sample LPIPS + the pooled gradient, then
    dge_space_loss_finalize_rows and dge_space_loss_bwd_rows.  `gb` (or None) is WRITTEN with sum_k weights[k] * d loss_k[sample]/db
    (need[k] False leaves window k out), `ga` (latents only) with the gradient w.r.t. a.  Returns out8 [B, nwin, 8]."""
    import ctypes as C
    B, Cc, H, W = a.shape
    dev = a.device
    L = lib()
    nw = len(wins)
    h0, w0 = wins[0][2], wins[0][3]
    nblk = max(1, min(256, (h0 * w0 + 1023) // 1024))
    wflat = (C.c_int * (4 * nw))(*[int(v) for win in wins for v in win])
    part = torch.empty((B, nw, nblk, 8), dtype=torch.float32, device=dev)
    check(L.dge_loss_reduce_rows(_f32(a), _f32(b), _p(part), B, Cc, H, W, wflat, nw, nblk, _stream()), "dge_loss_reduce_rows")
    ops.log_kernel()
    ks = [_pool_factor(win[2]) if image_space else 1 for win in wins]
    ns = [float(Cc * win[2] * win[3]) for win in wins]
    npools = [float(Cc * (win[2] // k) * (win[3] // k)) for win, k in zip(wins, ks)]
    tiles, lps, gps = [None] * nw, [None] * nw, [None] * nw
    want = [bool(gb is not None and need[i]) for i in range(nw)]
    if image_space:
        aps = [torch.empty((B, Cc, win[2] // k, win[3] // k), dtype=torch.float32, device=dev) for win, k in zip(wins, ks)]
        bps = [torch.empty_like(t) for t in aps]
        srcs = (C.c_void_p * (2 * nw))(*([a.data_ptr()] * nw + [b.data_ptr()] * nw))
        dsts = (C.c_void_p * (2 * nw))(*([t.data_ptr() for t in aps] + [t.data_ptr() for t in bps]))
        w2 = (C.c_int * (8 * nw))(*([int(v) for win in wins for v in win] * 2))
        k2 = (C.c_int * (2 * nw))(*(ks * 2))
        check(L.dge_crop_pool_multi(srcs, dsts, w2, k2, 2 * nw, B * Cc, H, W, _stream()), "dge_crop_pool_multi")
        main, side = _window_streams(dev, lpips_model, nw, B * H * W)       # the windows' LPIPS launches fork as in _space_loss_windows3
        for i in range(nw):
            ap, bp = aps[i], bps[i]
            hp, wp = ap.shape[2], ap.shape[3]
            strm = side[i - 1] if (side and i > 0) else None
            if strm is not None:
                strm.wait_stream(main)
            with (torch.cuda.stream(strm) if strm is not None else contextlib.nullcontext()):
                dmap = torch.empty((3, B, Cc, hp, wp), dtype=torch.float32, device=dev) if want[i] else None
                tiles[i] = torch.empty((B, Cc * ((hp + 15) // 16) * ((wp + 15) // 16)), dtype=torch.float32, device=dev)
                check(L.dge_ssim_fwd_rows(_p(ap), _p(bp), _p(tiles[i]), _p(dmap), B * Cc, hp, wp, _stream()), "dge_ssim_fwd_rows")
                ops.log_kernel()
                g_lp = None
                if lpips_model is not None:
                    lps[i], g_lp = lpips_model.value_and_grad(ap, bp, need_grad=want[i], per_sample=True)
                if want[i]:
                    gps[i] = torch.empty_like(bp)
                    check(L.dge_ssim_bwd(_p(ap), _p(bp), _p(dmap), _p(gps[i]), B * Cc, hp, wp, -1.0 / npools[i], 0, _stream()), "dge_ssim_bwd")
                    if g_lp is not None:      # g_lp = d mean_b lpips / db = (1/B) d lpips[sample] / db; the loss holds 2 * lpips[sample]
                        check(L.dge_axpy_scalar(_p(g_lp), None, _p(gps[i]), g_lp.numel(), 2.0 * B, 1, _stream()), "dge_axpy_scalar")
            if strm is not None:            # results allocated on the side stream are read (and freed) under the caller's stream
                for t in (dmap, tiles[i], lps[i], g_lp, gps[i]):
                    if t is not None:
                        t.record_stream(main)
        for strm in side:
            main.wait_stream(strm)
        if lpips_model is not None:
            lpips_model._streams_warm = True
    ptrs = lambda ts: (C.c_void_p * nw)(*[(t.data_ptr() if t is not None else None) for t in ts])
    sums7 = torch.empty((B, nw, 8), dtype=torch.float32, device=dev)
    out8 = torch.empty((B, nw, 8), dtype=torch.float32, device=dev)
    cnt = (C.c_int * nw)(*[(t.shape[1] if t is not None else 0) for t in tiles])
    nn, pp = (C.c_float * nw)(*ns), (C.c_float * nw)(*npools)
    check(L.dge_space_loss_finalize_rows(_p(part), nblk, ptrs(tiles) if image_space else None, cnt if image_space else None,
                                         ptrs(lps) if image_space else None, _p(sums7), _p(out8), B, nw, nn, pp, 1 if image_space else 0,
                                         _stream()), "dge_space_loss_finalize_rows")
    ops.log_kernel()
    kk = (C.c_int * nw)(*ks)
    if gb is not None:
        ww = (C.c_float * nw)(*[float(weights[i]) if want[i] else 0.0 for i in range(nw)])
        check(L.dge_space_loss_bwd_rows(_f32(a), _f32(b), _p(sums7), ptrs(gps) if image_space else None, _p(gb), B, Cc, H, W, wflat, kk,
                                        nn, ww, nw, 0, _stream()), "dge_space_loss_bwd_rows")
        ops.log_kernel()
    if ga is not None:
        ww = (C.c_float * nw)(*[float(weights[i]) for i in range(nw)])
        check(L.dge_space_loss_bwd_rows(_f32(b), _f32(a), _p(sums7), None, _p(ga), B, Cc, H, W, wflat, kk, nn, ww, nw, 1, _stream()),
              "dge_space_loss_bwd_rows")
        ops.log_kernel()
    return out8


def _no_global_batch(global_batch, what):
    if global_batch is not None:
        raise ValueError(f"{what} is not offered with global_batch: the samples of a data-parallel batch are independent already")


def image_loss_tsa_rows(imgs1, imgs2, lpips_model=None, weights=(1.0, 5.0, 9.0), grad_windows=(True, True, True), global_batch=None):
    """image_loss_tsa with every sample a loss of its own: loss_b is image_loss_tsa(imgs1[b:b+1], imgs2[b:b+1], ...).  Returns
    (sum_b loss_b on device, carrying the analytic gradient - row b of it is d loss_b / d imgs2[b] -, info [B,3,8] on device: per
    sample the rows and columns of image_loss_tsa's info).  The same kernels and bits in both reduction modes.  No host
    synchronisation."""
    _no_global_batch(global_batch, "image_loss_tsa_rows")
    a = imgs1.detach().float().contiguous()
    b = imgs2.detach().float().contiguous()
    need = imgs2.requires_grad and torch.is_grad_enabled()
    wins = attention_windows(a.shape[2], a.shape[3])
    g = torch.empty_like(b) if need else None
    info = _space_loss_rows(a, b, wins, True, lpips_model, weights, [bool(need and grad_windows[i]) for i in range(3)], gb=g)
    loss = (info[:, 0, 0] * float(weights[0]) + info[:, 1, 0] * float(weights[1]) + info[:, 2, 0] * float(weights[2])).sum()
    if need:
        loss = _ScaledGrad.apply(imgs2, loss, g)
    return loss, info


def space_loss_rows(imgs1, imgs2, image_space=False, global_batch=None):
    """space_loss on latents with every sample a loss of its own: loss_b is space_loss(imgs1[b:b+1], imgs2[b:b+1],
    image_space=False) - one row is its own cosine vector and its own softmax group, whatever its rank.  Returns (sum_b loss_b on
    device with the analytic gradient of both arguments attached where they carry one, info [B,8]).  No host synchronisation."""
    _no_global_batch(global_batch, "space_loss_rows")
    if image_space:
        raise ValueError("space_loss_rows: latents only (images go through image_loss_tsa_rows)")
    a = imgs1.detach().float().contiguous()
    b = imgs2.detach().float().contiguous()
    Bt = a.shape[0]
    n_in = a.numel() // Bt
    grad = torch.is_grad_enabled()
    need_a, need_b = imgs1.requires_grad and grad, imgs2.requires_grad and grad
    ga = torch.empty_like(a) if need_a else None
    gb = torch.empty_like(b) if need_b else None
    view = lambda t: t.view(Bt, 1, 1, n_in) if t is not None else None
    info = _space_loss_rows(view(a), view(b), [(0, 0, 1, n_in)], False, None, [1.0], [True], ga=view(ga), gb=view(gb))[:, 0]
    loss = info[:, 0].sum()
    if need_a:
        loss = _ScaledGrad2.apply(imgs1, imgs2, loss, ga, gb if need_b else torch.zeros_like(b))
    elif need_b:
        loss = _ScaledGrad.apply(imgs2, loss, gb)
    return loss, info

