"""Which launcher a StyleGAN2 ModulateConvBlock `L` runs on, and with which packed copy of its weight.  The route of a layer is a
value, decided before anything is launched by `forward_route` / `dgrad_route` - the two ordered rule lists, each rule with the
measurement behind it - from the layer's shape, the batch, the dtype, the mode and the switches below; `forward` / `dgrad` look the
route up and run its launcher (FORWARD / DGRAD), and every launcher owns the packed weight copy its kernel reads.  The switches
(A/B measurements) are read from the environment once, at import, and from this module at every call."""
import collections
import os

from . import ops
from .weight_cache import lookup, store

PP_GEN = not os.environ.get("DGE_NO_PP_GEN")
UP_PP = os.environ.get("DGE_UP_PP", "1") != "0"      # round 6: the default for the Cin >= 128 up layers (dge_up_pp: up_s4 / up_pp kernels; DGE_UP_PP=0: upconv_fir)
UP_FOLDED = os.environ.get("DGE_UP_FOLDED") == "1"
T2D = not os.environ.get("DGE_NO_T2D")
PP_DG = not os.environ.get("DGE_NO_PP_DG")
UP_DG_STREAM = not os.environ.get("DGE_NO_UP_DG_STREAM")      # the 64 <- 32 up layer's data gradient as one streaming launch (csrc/upconv_stream_bwd.hip)
UP_DG_SMALL = not os.environ.get("DGE_NO_UP_DG_SMALL")        # the 512-channel up layers at <= 32^2: phase-form data gradient on the low-resolution kernel (csrc/conv_small.hip)

# What the route rules read of a layer: a ModulateConvBlock has these attributes, and a LayerShape asks the rules without one.
LayerShape = collections.namedtuple("LayerShape", "up res in_c out_c ksize demodulate", defaults=(3, True))
ForwardRoute = collections.namedtuple("ForwardRoute", "kind")                # kind: a key of FORWARD
DgradRoute = collections.namedtuple("DgradRoute", "kind takes_prep")         # kind: a key of DGRAD; takes_prep: see dgrad_route


def _grid(L):
    """side of the grid the layer reads (= the grid its data-gradient conv runs on: the space-to-depth / t grid of an up layer)"""
    return L.res // 2 if L.up else L.res


def _cached(L, key, build):
    """the derived weight `key` of L, rebuilt only when the parameter changes"""
    c = lookup(L._cache, key, L.weight)
    return c if c is not None else store(L._cache, key, L.weight, build())


# ------------------------------------------------------------------ forward
def forward_route(L, B, dtype, rgb=False):
    """Route of the modulated conv of layer L (shape record or block) at batch B; `rgb`: the launch also writes the toRGB of its
    result.  First match wins.  (Both callers - synthesis_run and ModulateConvBlock.forward - pass the style and, for a demodulating
    layer, the demodulation factor, and one noise strength per layer; the tests of the earlier chain for a missing scale or a
    per-channel strength could not fail and are gone.)"""
    h = _grid(L)
    # phase-form up kernels ([9 units][Cout][Cin] weights).  Input resolutions below 16: a single 16x16 t-pixel tile per sample would
    # be mostly padding - the folded 3x3-per-phase form of conv2d(up=True) is faster
    if L.up and L.res >= 32 and not UP_FOLDED and ops.upconv_supported(L.in_c, L.out_c, dtype):
        # MFMA-bound up layers (Cin >= 128): fused modulation (:858-875) folded into one weight image per sample, ping-pong
        # implicit GEMM with the FIR in registers (csrc/up_pp.hip)
        if UP_PP and L.demodulate and ops.up_pp_supported(B, h, h, L.in_c, L.out_c, dtype):
            return ForwardRoute("up_pp")
        return ForwardRoute("upconv_fir")
    # MFMA-bound layers (>= 128 channels at 64^2 .. 256^2): the reference's fused modulation (:858-875) - style, demodulation
    # and gain folded into one weight image per sample - feeding the ping-pong implicit GEMM (csrc/conv_pp.hip)
    if PP_GEN and not rgb and not L.up and L.demodulate and L.ksize == 3 and ops.conv_pp_supported(B, h, h, L.in_c, L.out_c, dtype):
        return ForwardRoute("conv_pp")
    return ForwardRoute("conv2d")


def prepared(L, dtype):
    """-- derived weights, rebuilt only when the parameter changes: (packed copy for conv2d, per-(o,i) sum of squares)"""
    def build():
        mode = ops.PACK_UPFOLD if L.up else ops.PACK_FWD
        hin = _grid(L)                               # the low-resolution layers get fragment-ordered weights (conv_small)
        packed = ops.pack_conv_weight(L.weight, ops.pack_mode_for(L.weight, mode, hin, hin, dtype), dtype, L.wscale) \
            if L.ksize == 3 else None
        return packed, (ops.weight_sumsq(L.weight, L.wscale) if L.demodulate else None)
    return _cached(L, ("w", dtype), build)


def _up_units(L, dt):
    """[9 units][Cout][Cin] weights of the phase-form up kernels"""
    return _cached(L, ("wu", dt), lambda: ops.pack_upconv_weight(L.weight, dt, L.wscale))


def _fw_up_pp(L, x, s, d, tail, dt, rgb):
    assert rgb is None
    wimg = ops.pack_up_pp(_up_units(L, dt), L.out_c, L.in_c, in_scale=s, out_scale=d, gain=L.gain)
    return ops.up_pp(x, wimg, L.out_c, **tail)


def _fw_upconv_fir(L, x, s, d, tail, dt, rgb):
    assert rgb is None
    return ops.upconv_fir(x, _up_units(L, dt), L.out_c, in_scale=s, out_scale=d, **tail)


def _fw_conv_pp(L, x, s, d, tail, dt, rgb):
    wpp = ops.pack_conv_pp(L.weight, L.wscale, in_scale=s, out_scale=d, gain=L.gain)
    return ops.conv_pp(x, wpp, L.out_c, **tail)


def _fw_conv2d(L, x, s, d, tail, dt, rgb):
    return ops.conv2d(x, prepared(L, dt)[0], L.out_c, 3, up=L.up, in_scale=s, out_scale=d, rgb=rgb, **tail)


FORWARD = {"up_pp": _fw_up_pp, "upconv_fir": _fw_upconv_fir, "conv_pp": _fw_conv_pp, "conv2d": _fw_conv2d}


def forward(L, x, s, d, noise, dt, rgb=None):
    """The modulated conv proper (:898-921) on NHWC activations: shared-weight form with s / d as prologue / epilogue scales.
    `rgb`: fused toRGB of the result (ops.conv2d), stride-1 layers only."""
    nw = L.noise_strength.detach().reshape(1) if noise is not None else None
    tail = dict(bias=L.bias, bias_scale=L.bscale, noise=noise, noise_w=nw, act=L.act, gain=L.gain)
    return FORWARD[forward_route(L, x.shape[0], dt, rgb is not None).kind](L, x, s, d, tail, dt, rgb)


# ------------------------------------------------------------------ data gradient
def dgrad_route(L, B, dtype, fused, pending_d):
    """Route of the data-gradient launch of layer L (shape record or block) at batch B.  `fused`: the atomics mode (not
    ops.is_deterministic()); `pending_d`: the incoming gradient is g_z with the layer's demodulation factor still to be applied (the
    tail backward of this layer rode the launch above) - the launch applies it in its prologue, or folds it into its weights.
    `takes_prep`: the launch carries the tail backward of the layer BELOW in its epilogue (the `prep` of ops.conv2d); only in
    atomics mode, whose sums leave by atomics.  First match wins.

    What autograd_s2.synthesis_backward, the one caller, can ask: deterministic mode never has pending_d, and in atomics mode
    pending_d is true for the top layer and below every layer that takes prep.  It builds `prep` exactly where takes_prep says so
    and a layer below exists (i >= 1) - up layers are odd layers, so an up layer whose route takes prep always gets it.  The chain
    this replaces tested three things that caller cannot vary, and they are gone: a missing dot_src / stats (it always passes out_scale,
    addend, stats and dot_src), further epilogue keywords, and `prep is not None` on the conv_pp phase form."""
    h = _grid(L)
    # Phase form (FIR^T pass + 4-tap conv on the t grid, dge_fir_t2d / in_t2d: 16 tap-units per input pixel instead of the 36 of the
    # folded space-to-depth form) for the MFMA-bound up layers, 32^2 .. 128^2 input (measured at batch 8, tools/perf_t2d.py, folded ->
    # FIR pass + conv: 512->512 @32^2 221 -> 174 us, 256<-512 @64^2 310 -> 243, 128<-256 @128^2 344 -> 313; at 256^2 / 512^2 the
    # launch is bound by its epilogue and the extra pass loses: 430 -> 504, 951 -> 1223).  On conv2d the small grids stay folded.
    t2d = bool(T2D and L.up and 32 <= h <= 128 and L.in_c >= 64 and L.in_c % 32 == 0 and L.out_c % 8 == 0)
    # The space-to-depth data gradient of a narrow up layer (layer 15: 64 -> 32 channels) loses more in its 64-wide conv_igemm tile
    # than the separate tail pass costs: measured 890 vs 747 us; tools/perf_prep.py
    takes_prep = bool(fused and (t2d or not (L.up and L.in_c < 128)))
    if fused and L.up and L.ksize == 3:
        # narrow up layer (64 <- 32, bf16): FIR^T, the 9-tap adjoint on the t grid and the epilogue in one streaming pass
        # (ops.up_dgrad_stream).  It carries the tail too: the stored activation of the layer below is in its registers anyway
        if UP_DG_STREAM and ops.up_dgrad_stream_supported(B, h, h, L.in_c, L.out_c, dtype):
            return DgradRoute("up_stream", True)
        # low-resolution up layers (256 / 512 channels out on a grid <= 32^2, bf16: 512 <- 512 at 4^2 .. 32^2): FIR^T to the t grid,
        # then the 9 non-zero units on the low-resolution kernel (ops.up_dgrad_small); deterministic mode and f32 keep their launches
        if UP_DG_SMALL and ops.up_dgrad_small_supported(B, h, h, L.in_c, L.out_c, dtype):
            return DgradRoute("up_small", takes_prep)
    # MFMA-bound launches on the ping-pong kernel (csrc/conv_pp.hip; GEMM K = out channels, x 4 phases for an up layer; N = in
    # channels).  Its sums leave by atomics
    if fused and PP_DG and (not L.up or L.out_c % 32 == 0) and ops.conv_pp_supported(B, h, h, (4 if L.up else 1) * L.out_c, L.in_c, dtype):
        if t2d:              # phase form: the same FIR^T pass, then the 4-tap conv with ONE shared weight image
            return DgradRoute("pp_t2d", takes_prep)
        if pending_d:        # the demodulation factor is folded into a per-sample weight image instead of scaling g_z in a prologue
            return DgradRoute("pp", takes_prep)
    return DgradRoute("t2d" if t2d else "igemm", takes_prep)


def dgrad_takes_prep(L, B, dtype):
    """True when the data-gradient launch of L carries the tail backward of the layer below in its epilogue (`prep`), in the mode
    the library is in"""
    return dgrad_route(L, B, dtype, not ops.is_deterministic(), True).takes_prep


def _conv2d_dgrad_weight(L, dt, mode):
    return _cached(L, ("dg", dt, mode), lambda: ops.pack_conv_weight(L.weight, mode, dt, L.wscale))


def _dg_igemm(L, g_y, d_in, dt, prep, ep):
    """conv2d on g_y; an up layer in the folded space-to-depth form"""
    mode = ops.pack_mode_for(L.weight, ops.PACK_UPFOLD_DGRAD if L.up else ops.PACK_DGRAD, _grid(L), _grid(L), dt)
    return ops.conv2d(g_y, _conv2d_dgrad_weight(L, dt, mode), L.in_c, 3, in_s2d=L.up, in_scale=d_in, add_scale=1.0, prep=prep, **ep)


def _dg_t2d(L, g_y, d_in, dt, prep, ep):
    """phase form: FIR^T (times the demodulation factor) to the t grid, then the 4-tap conv"""
    return ops.conv2d(ops.fir_t2d(g_y, d_in), _conv2d_dgrad_weight(L, dt, ops.PACK_UPT2D_DGRAD), L.in_c, 3, in_t2d=True, add_scale=1.0,
                      prep=prep, **ep)


def _dg_pp(L, g_y, d_in, dt, prep, ep):
    """per sample, W'[b] = bf16(w * wscale * d[b, o]); the up layer through its folded f32 rows, packed once per weight version"""
    if L.up:
        rows = _cached(L, "dgpp", lambda: ops.pack_conv_weight(L.weight, ops.PACK_UPFOLD_DGRAD, ops.F32, L.wscale))
        w = ops.pack_conv_pp_rows(rows, L.in_c, in_scale=d_in, in_period=L.out_c)
    else:
        w = ops.pack_conv_pp(L.weight, L.wscale, in_scale=d_in, dgrad=True)
    return ops.conv_pp(g_y, w, L.in_c, dgrad=True, in_s2d=L.up, add_scale=1.0, prep=prep, **ep)


def _dg_pp_t2d(L, g_y, d_in, dt, prep, ep):
    """one shared 4-tap image, cached per weight version"""
    def build():
        return ops.pack_conv_pp_rows(ops.pack_conv_weight(L.weight, ops.PACK_UPT2D_DGRAD, ops.F32, L.wscale), L.in_c, t2d=True)
    return ops.conv_pp(ops.fir_t2d(g_y, d_in), _cached(L, "dgpp_t2d", build), L.in_c, dgrad=True, in_t2d=True, add_scale=1.0, prep=prep, **ep)


def _dg_up_stream(L, g_y, d_in, dt, prep, ep):
    w = _cached(L, ("dgs", dt), lambda: ops.pack_up_dgrad_stream(L.weight, dt, L.wscale))
    return ops.up_dgrad_stream(g_y, w, d_in, ep["out_scale"], ep["addend"], ep["stats"], ep["dot_src"], prep=prep)


def _dg_up_small(L, g_y, d_in, dt, prep, ep):
    z = ops.fir_t2d(g_y, d_in)
    w = _cached(L, ("dgu", dt), lambda: ops.pack_up_dgrad_small(L.weight, dt, L.wscale))
    return ops.up_dgrad_small(z, w, ep["out_scale"], ep["addend"], ep["stats"], ep["dot_src"], prep=prep)


DGRAD = {"up_stream": _dg_up_stream, "up_small": _dg_up_small, "pp": _dg_pp, "pp_t2d": _dg_pp_t2d, "t2d": _dg_t2d, "igemm": _dg_igemm}


def dgrad(L, route, g_y, d_in, dt, prep, out_scale, addend, stats, dot_src):
    """g_xprev [B,Hin,Win,in_c] of layer L from g_y on `route` (dgrad_route with pending_d = d_in is not None); d_in: the
    demodulation factor still to be applied to g_y, or None.  `prep` (where route.takes_prep) and the epilogue operands go to the
    launch as they are (ops.conv2d / ops.conv_pp)."""
    return DGRAD[route.kind](L, g_y, d_in, dt, prep, dict(out_scale=out_scale, addend=addend, stats=stats, dot_src=dot_src))
