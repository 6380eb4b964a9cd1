"""space_loss (reference training_utils.py:54-99) and the three-scale image loss of
E_align_s2.py:185-203 on the HIP kernels, as autograd Functions whose forward also produces the
analytic gradient w.r.t. the second argument (the only one that carries grad in E_align).

Every form walks its one to three nested windows through the same middle, _pooled_stage: one dge_crop_pool_multi launch, then per
window SSIM, LPIPS value and gradient and the pooled-image gradient, forked to side streams where that pays.  Around it there are
two ends.  _coupled_losses: the sums run over the (global) batch - dge_loss_reduce3 or dge_loss_reduce per window, one exchange of
the packed sums, dge_space_loss_finalize; the gradient is one of _bwd3 (image_loss_tsa), _bwd_each (space_loss, and
image_loss_tsa in deterministic mode) and _bwd_split (image_losses_split).  _rows_losses: the per-sample forms image_loss_tsa_rows
/ space_loss_image_rows / space_loss_rows (embedding_v2 `independent`, embedding_v2_biggan.BigEmbedRowsStep): sample b's loss is
what image_loss_tsa / space_loss return on the one-row slices, the result is their sum over b (so the gradient of row b is the gradient of its own loss) and the info tensors keep a row per
sample."""
import contextlib
import ctypes as C
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


# ------------------------------------------------------------------ ctypes tables of the multi-window entry points
def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[(t.data_ptr() if t is not None else None) for t in ts])


def _ints(vs):
    return (C.c_int * len(vs))(*vs)


def _floats(vs):
    return (C.c_float * len(vs))(*vs)


def _wflat(wins):
    return _ints([int(v) for win in wins for v in win])


# ------------------------------------------------------------------ the pooled stage (all forms)
class _Win:
    """What the ends need of one window: the pooled images ap, bp and the pooling factor k, the element counts n / npool the means
    of the full-size / pooled terms run over, the LPIPS value lp, the pooled-image gradient gp (SSIM + LPIPS; None: no gradient).
    sums (coupled forms): the window's 8 sums in the packed buffer; tiles (rows form): its SSIM tile sums per sample."""
    __slots__ = ("ap", "bp", "k", "n", "npool", "lp", "gp", "sums", "tiles")

    def __init__(self, win, k, planes):
        self.k = k
        self.n, self.npool = float(planes * win[2] * win[3]), float(planes * (win[2] // k) * (win[3] // k))
        self.ap = self.bp = self.lp = self.gp = self.sums = self.tiles = None


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


def _pooled_stage(a, b, wins, ks, lpips_model, want, planes, pack=None, world=1):
    """The pooled part of space_loss on the windows `wins` of a, b [B,C,H,W], pooled by `ks`: one dge_crop_pool_multi launch for the
    2 * nwin pooled images, then per window SSIM forward, LPIPS value and gradient and, where want[i], the pooled-image gradient
    gp = d(1 - ssim + 2 * lpips)/d bp (neither term needs the global sums).  Returns a _Win per window.
    Coupled forms: `pack` is their [nwin, _PK] buffer - window i's SSIM slot copies go to pack[i, 8:40], its LPIPS mean (world > 1:
    the rank's share of the global mean) to pack[i, 40:41]; `planes` = B * C * world.  Rows form (pack None): SSIM tile sums and
    LPIPS values per sample, `planes` = C."""
    B, Cc, H, W = a.shape
    dev = a.device
    L = lib()
    nw = len(wins)
    rows = pack is None
    # d lpips / d bp as value_and_grad returns it is that of the batch MEAN: the rows form holds 2 * lpips[sample] = 2 * B * its share
    lp_scale = 2.0 * B if rows else 2.0 / world
    aps = [torch.empty((B, Cc, win[2] // k, win[3] // k), dtype=torch.float32, device=dev) for win, k in zip(wins, ks)]
    bps = [torch.empty_like(t) for t in aps]
    check(L.dge_crop_pool_multi(_ptrs([a] * nw + [b] * nw), _ptrs(aps + bps), _wflat(list(wins) * 2), _ints(list(ks) * 2), 2 * nw, B * Cc,
                                H, W, _stream()), "dge_crop_pool_multi")
    # The windows are independent from here to the join below, and their LPIPS launches are small (conv3 - conv5 on 16^2 .. 64^2
    # features: 256 - 1152 workgroups, one or two per CU, each a serial weight stream): on one stream they run one after the
    # other on a half-empty chip.  Each window gets its own stream (forked off the caller's, joined before the results are
    # read); the first call stays on one stream (it fills the LPIPS weight-pack cache), so does the deterministic mode (its
    # slot workspace belongs to one stream at a time).
    main, side = _window_streams(dev, lpips_model, nw, B * H * W)
    sts = []
    for i, win in enumerate(wins):
        st = _Win(win, ks[i], planes)
        ap, bp = st.ap, st.bp = aps[i], bps[i]
        hp, wp = ap.shape[2], ap.shape[3]
        strm = side[i - 1] if (side and i > 0) else None
        if strm is not None:
            strm.wait_stream(main)
        with (torch.cuda.stream(strm) if strm is not None else contextlib.nullcontext()):
            dmap = torch.empty((3, B, Cc, hp, wp), dtype=torch.float32, device=dev) if want[i] else None
            g_lp = None
            if rows:
                st.tiles = torch.empty((B, Cc * ((hp + 15) // 16) * ((wp + 15) // 16)), dtype=torch.float32, device=dev)
                check(L.dge_ssim_fwd_rows(_p(ap), _p(bp), _p(st.tiles), _p(dmap), B * Cc, hp, wp, _stream()), "dge_ssim_fwd_rows")
                ops.log_kernel()
                if lpips_model is not None:
                    st.lp, g_lp = lpips_model.value_and_grad(ap, bp, need_grad=want[i], per_sample=True)
            else:
                # pack[i, 8:40]: 32 slot copies of the SSIM sum (atomics contention), added up by the finaliser
                check(L.dge_ssim_fwd(_p(ap), _p(bp), _p(pack[i, 8:40]), _p(dmap), B * Cc, hp, wp, _stream()), "dge_ssim_fwd")
                if lpips_model is not None:
                    st.lp, g_lp = lpips_model.value_and_grad(ap, bp, need_grad=want[i])      # mean over the rank's batch, d/dbp
                    if world > 1:      # global mean = sum over ranks of (rank mean / world): joins the packed exchange
                        check(L.dge_axpy_scalar(_p(st.lp), None, _p(pack[i, 40:41]), 1, 1.0 / world, 0, _stream()), "dge_axpy_scalar")
                        st.lp = pack[i, 40:41]
            if want[i]:
                st.gp = torch.empty_like(bp)
                check(L.dge_ssim_bwd(_p(ap), _p(bp), _p(dmap), _p(st.gp), B * Cc, hp, wp, -1.0 / st.npool, 0, _stream()), "dge_ssim_bwd")
                if g_lp is not None:
                    check(L.dge_axpy_scalar(_p(g_lp), None, _p(st.gp), g_lp.numel(), lp_scale, 1, _stream()), "dge_axpy_scalar")
        if strm is not None:            # results allocated on the side stream are read (and freed) under the caller's stream
            for t in (dmap, st.tiles, st.lp, g_lp, st.gp):
                if t is not None:
                    t.record_stream(main)
        sts.append(st)
    for strm in side:
        main.wait_stream(strm)
    # the next call may fork: this one ran the LPIPS kernels of a forking call on one stream (the rows form runs the same ones in
    # both reduction modes, the coupled forms fork - and mark - only outside the deterministic mode)
    if lpips_model is not None and nw > 1 and (rows or not ops.is_deterministic()):
        lpips_model._streams_warm = True
    return sts


# ------------------------------------------------------------------ coupled forms: the sums run over the (global) batch
def batch_sums(a, b, win, out=None):
    """The 8 sums of dge_loss_reduce over window `win` of a, b [B,C,H,W]: 16 slot copies (atomics contention), added up into `out`
    (pre-zeroed) or a new [8] tensor."""
    B, Cc, H, W = a.shape
    slots = ops.zeros((16, 8), a.device)
    check(lib().dge_loss_reduce(_f32(a), _f32(b), _p(slots), B, Cc, H, W, *win, _stream()), "dge_loss_reduce")
    return ops._sum_over_batch(slots, out)


def _coupled_losses(a, b, wins, image_space, lpips_model, want, gb=None):
    """space_loss on the windows `wins` of a, b [B,C,H,W] (training_utils.py:54-99 each) up to the loss terms: every per-rank partial
    sum goes into one packed buffer, a data-parallel run (`gb`) exchanges ALL windows in one all-reduce, then the finaliser runs
    per window.  Several windows take every image pass merged (dge_loss_reduce3; not offered in deterministic mode, which reduces
    window by window).  Returns (a _Win per window for the gradient, the list of out8 tensors)."""
    B, Cc, H, W = a.shape
    dev = a.device
    L = lib()
    nw = len(wins)
    world = gb.world if gb is not None else 1
    pack = ops.zeros((nw, _PK), dev)
    if nw > 1 and not ops.is_deterministic():
        slots = ops.zeros((nw, 16, 8), dev)
        check(L.dge_loss_reduce3(_f32(a), _f32(b), _p(slots), B, Cc, H, W, _wflat(wins), nw, _stream()), "dge_loss_reduce3")
        sums = ops.DeferredSums()
        for i in range(nw):
            sums.add(slots[i].view(16, 8, 1), pack[i, 0:8])      # [nslot, C = 8, NS = 1] -> the 8 sums of window i
        sums.flush()
    else:
        for i, win in enumerate(wins):
            batch_sums(a, b, win, pack[i, 0:8])
    if image_space:
        sts = _pooled_stage(a, b, wins, [_pool_factor(win[2]) for win in wins], lpips_model, want, B * Cc * world, pack, world)
    else:
        sts = [_Win(win, 1, B * Cc * world) for win in wins]
    if gb is not None:
        gb.reduce(pack)
    outs = []
    for i, st in enumerate(sts):
        st.sums = pack[i, 0:8]
        out8 = torch.empty(8, dtype=torch.float32, device=dev)
        check(L.dge_space_loss_finalize(_p(st.sums), _p(pack[i, 8:40]) if image_space else None, _p(st.lp), _p(out8), st.n, st.npool,
                                        1 if image_space else 0, _stream()), "dge_space_loss_finalize")
        outs.append(out8)
    return sts, outs


def _bwd_each(a, b, wins, sts, weights, want, g, accumulate):
    """dge_space_loss_bwd per wanted window: weights[k] * (window k's gradient) is written into that window of g, or added to it."""
    B, Cc, H, W = a.shape
    for win, st, wt, on in zip(wins, sts, weights, want):
        if on:
            check(lib().dge_space_loss_bwd(_f32(a), _f32(b), _p(st.sums), _p(st.gp), _p(g), B * Cc, H, W, *win, st.k, st.n, float(wt),
                                           1 if accumulate else 0, _stream()), "dge_space_loss_bwd")


def _bwd_tables(a, wins, sts, weights, want):
    """The arguments dge_space_loss_bwd3 and dge_space_loss_bwd_split share, before and after the gradient image(s)"""
    B, Cc, H, W = a.shape
    wts = [float(wt) if on else 0.0 for wt, on in zip(weights, want)]
    return ((_ptrs([st.sums for st in sts]), _ptrs([st.gp for st in sts])),
            (B * Cc, H, W, _wflat(wins), _ints([st.k for st in sts]), _floats([st.n for st in sts]), _floats(wts), len(wins), _stream()))


def _bwd3(a, b, wins, sts, weights, want, g):
    """One dge_space_loss_bwd3 launch: g is WRITTEN with the weighted sum of the wanted windows' gradients."""
    src, dims = _bwd_tables(a, wins, sts, weights, want)
    check(lib().dge_space_loss_bwd3(_f32(a), _f32(b), *src, _p(g), *dims), "dge_space_loss_bwd3")


def _bwd_split(a, b, wins, sts, weights, want, outs):
    """One dge_space_loss_bwd_split launch: outs[k] (or None) is WRITTEN with weights[k] * (window k's gradient), zeros outside it."""
    if all(t is None for t in outs):
        return
    src, dims = _bwd_tables(a, wins, sts, weights, want)
    check(lib().dge_space_loss_bwd_split(_f32(a), _f32(b), *src, _ptrs(outs), *dims), "dge_space_loss_bwd_split")
    ops.log_kernel()


def _space_loss_window(a, b, win, image_space, lpips_model, g, gb=None):
    """space_loss on one window of a, b [B,C,H,W]; g (or None) is WRITTEN with dloss/db.  Returns out8."""
    want = [g is not None]
    sts, outs = _coupled_losses(a, b, [win], image_space, lpips_model, want, gb)
    _bwd_each(a, b, [win], sts, [1.0], want, g, accumulate=False)
    return outs[0]


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
    want = [bool(need and grad_windows[i]) for i in range(3)]
    det = ops.is_deterministic()
    g = (torch.zeros_like(b) if det else torch.empty_like(b)) if need else None
    sts, infos = _coupled_losses(a, b, wins, True, lpips_model, want, global_batch)
    if need and det:          # (dge_space_loss_bwd3's 16-byte form multiplies by reciprocals: not the bits of the single-window kernel)
        _bwd_each(a, b, wins, sts, weights, want, g, accumulate=True)
    elif need:
        _bwd3(a, b, wins, sts, weights, want, g)
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
    sts, infos = _coupled_losses(a, b, wins, True, lpips_model, want, global_batch)
    _bwd_split(a, b, wins, sts, weights, want, gs)
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
        out8 = _space_loss_window(a, b, (0, 0, H, W), True, lpips_model, g, gb=global_batch)
    else:
        # 3-D latents: the implicit softmax dim is 0 (the batch) -> planes = batch (training_utils.py:67)
        Bt = a.shape[0]
        n_in = a.numel() // Bt
        if a.dim() == 2:
            # 2-D latents (PGGAN / BigGAN z): the implicit softmax dim is 1 -> one softmax per sample over the features
            out8 = _space_loss_window(a.view(Bt, n_in, 1, 1), b.view(Bt, n_in, 1, 1), (0, 0, 1, 1), False, None,
                                      g.view(Bt, n_in, 1, 1) if need else None, gb=global_batch)
            loss = out8[0]
            if imgs1.requires_grad and torch.is_grad_enabled():
                # the first argument carries a gradient too (embedding_v2_biggan: w1 is the optimised leaf or the encoder's output):
                # the exchanged call, as for 3-D latents below
                ga = torch.empty_like(a)
                _space_loss_window(b.view(Bt, n_in, 1, 1), a.view(Bt, n_in, 1, 1), (0, 0, 1, 1), False, None, ga.view(Bt, n_in, 1, 1),
                                   gb=global_batch)
                return _ScaledGrad2.apply(imgs1, imgs2, loss, ga, g if need else torch.zeros_like(b)), out8
            return (_ScaledGrad.apply(imgs2, loss, g) if need else loss), out8
        out8 = _space_loss_window(a.view(1, Bt, 1, n_in), b.view(1, Bt, 1, n_in), (0, 0, 1, n_in), False, None,
                                  g.view(1, Bt, 1, n_in) if need else None, gb=global_batch)
        if imgs1.requires_grad and torch.is_grad_enabled():
            # the first argument carries a gradient too: 5*mse + 3*cos is symmetric, so d/da is the same kernel with
            # the arguments exchanged (the logged-only KL term is not, and is taken from the first evaluation)
            ga = torch.empty_like(a)
            _space_loss_window(b.view(1, Bt, 1, n_in), a.view(1, Bt, 1, n_in), (0, 0, 1, n_in), False, None,
                               ga.view(1, Bt, 1, n_in), gb=global_batch)
            gbt = g if need else torch.zeros_like(b)
            return _ScaledGrad2.apply(imgs1, imgs2, out8[0], ga, gbt), out8
    loss = out8[0]
    if need:
        loss = _ScaledGrad.apply(imgs2, loss, g)
    return loss, out8


# ------------------------------------------------------------------ per-sample forms
def _rows_losses(a, b, wins, image_space, lpips_model, weights, need, ga=None, gb=None):
    """space_loss of every sample of a, b [B,C,H,W] on up to 3 nested windows (all inside window 0), the samples kept apart:
    dge_loss_reduce_rows, the pooled stage in its rows form (images only), then dge_space_loss_finalize_rows and
    dge_space_loss_bwd_rows.  `gb` (or None) is WRITTEN with sum_k weights[k] * d loss_k[sample]/db (need[k] False leaves window k
    out), `ga` (latents only) with the gradient w.r.t. a.  Returns out8 [B, nwin, 8]."""
    B, Cc, H, W = a.shape
    dev = a.device
    L = lib()
    nw = len(wins)
    h0, w0 = wins[0][2], wins[0][3]
    nblk = max(1, min(256, (h0 * w0 + 1023) // 1024))
    wflat = _wflat(wins)
    part = torch.empty((B, nw, nblk, 8), dtype=torch.float32, device=dev)
    check(L.dge_loss_reduce_rows(_f32(a), _f32(b), _p(part), B, Cc, H, W, wflat, nw, nblk, _stream()), "dge_loss_reduce_rows")
    ops.log_kernel()
    want = [bool(gb is not None and need[i]) for i in range(nw)]
    tiles = cnt = lps = gps = None
    if image_space:
        sts = _pooled_stage(a, b, wins, [_pool_factor(win[2]) for win in wins], lpips_model, want, Cc)
        tiles, lps, gps = _ptrs([st.tiles for st in sts]), _ptrs([st.lp for st in sts]), _ptrs([st.gp for st in sts])
        cnt = _ints([st.tiles.shape[1] for st in sts])
    else:
        sts = [_Win(win, 1, Cc) for win in wins]
    sums7 = torch.empty((B, nw, 8), dtype=torch.float32, device=dev)
    out8 = torch.empty((B, nw, 8), dtype=torch.float32, device=dev)
    nn, kk = _floats([st.n for st in sts]), _ints([st.k for st in sts])
    check(L.dge_space_loss_finalize_rows(_p(part), nblk, tiles, cnt, lps, _p(sums7), _p(out8), B, nw, nn, _floats([st.npool for st in sts]),
                                         1 if image_space else 0, _stream()), "dge_space_loss_finalize_rows")
    ops.log_kernel()
    if gb is not None:
        ww = _floats([float(weights[i]) if want[i] else 0.0 for i in range(nw)])
        check(L.dge_space_loss_bwd_rows(_f32(a), _f32(b), _p(sums7), gps, _p(gb), B, Cc, H, W, wflat, kk, nn, ww, nw, 0, _stream()),
              "dge_space_loss_bwd_rows")
        ops.log_kernel()
    if ga is not None:
        ww = _floats([float(weights[i]) for i in range(nw)])
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
    info = _rows_losses(a, b, wins, True, lpips_model, weights, [bool(need and grad_windows[i]) for i in range(3)], gb=g)
    loss = (info[:, 0, 0] * float(weights[0]) + info[:, 1, 0] * float(weights[1]) + info[:, 2, 0] * float(weights[2])).sum()
    if need:
        loss = _ScaledGrad.apply(imgs2, loss, g)
    return loss, info


def space_loss_image_rows(imgs1, imgs2, lpips_model=None, global_batch=None):
    """space_loss on images [B,3,H,W] or maps [B,1,H,W] with every sample a loss of its own: loss_b is space_loss(imgs1[b:b+1],
    imgs2[b:b+1], lpips_model=...) - the full window alone, with LPIPS (embedding_v2_biggan.BigEmbedRowsStep).  Returns (sum_b loss_b
    on device, carrying the analytic gradient - row b of it is d loss_b / d imgs2[b] -, info [B,8] on device).  The same kernels and
    bits in both reduction modes.  No host synchronisation."""
    _no_global_batch(global_batch, "space_loss_image_rows")
    if imgs1.dim() != 4:
        raise ValueError(f"space_loss_image_rows: images [B,C,H,W], got {tuple(imgs1.shape)} (latents go through space_loss_rows)")
    a = imgs1.detach().float().contiguous()
    b = imgs2.detach().float().contiguous()
    need = imgs2.requires_grad and torch.is_grad_enabled()
    g = torch.empty_like(b) if need else None
    info = _rows_losses(a, b, [(0, 0, a.shape[2], a.shape[3])], True, lpips_model, [1.0], [need], gb=g)[:, 0]
    loss = info[:, 0].sum()
    if need:
        loss = _ScaledGrad.apply(imgs2, loss, g)
    return loss, info


def space_loss_rows(imgs1, imgs2, image_space=False, global_batch=None):
    """space_loss on latents with every sample a loss of its own: loss_b is space_loss(imgs1[b:b+1], imgs2[b:b+1],
    image_space=False) - one row is its own cosine vector and its own softmax group (2-D latents: a softmax over the row's
    features).  Returns (sum_b loss_b on device with the analytic gradient of both arguments attached where they carry one, info
    [B,8]).  No host synchronisation."""
    _no_global_batch(global_batch, "space_loss_rows")
    if image_space:
        raise ValueError("space_loss_rows: latents only (images go through image_loss_tsa_rows / space_loss_image_rows)")
    a = imgs1.detach().float().contiguous()
    b = imgs2.detach().float().contiguous()
    Bt = a.shape[0]
    n_in = a.numel() // Bt
    grad = torch.is_grad_enabled()
    need_a, need_b = imgs1.requires_grad and grad, imgs2.requires_grad and grad
    ga = torch.empty_like(a) if need_a else None
    gb = torch.empty_like(b) if need_b else None
    # 2-D latents (BigGAN's w [B,128]): the implicit softmax dim of a one-row slice is 1, the features - they are the planes of a
    # one-pixel sample, as in space_loss; every other rank: the slice's softmax runs over its batch of one (one plane)
    shape, win = ((Bt, n_in, 1, 1), (0, 0, 1, 1)) if a.dim() == 2 else ((Bt, 1, 1, n_in), (0, 0, 1, n_in))
    view = lambda t: t.view(shape) if t is not None else None
    info = _rows_losses(view(a), view(b), [win], False, None, [1.0], [True], ga=view(ga), gb=view(gb))[:, 0]
    loss = info[:, 0].sum()
    if need_a:
        loss = _ScaledGrad2.apply(imgs1, imgs2, loss, ga, gb if need_b else torch.zeros_like(b))
    elif need_b:
        loss = _ScaledGrad.apply(imgs2, loss, gb)
    return loss, info

