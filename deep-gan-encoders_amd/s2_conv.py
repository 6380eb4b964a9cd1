"""Which launcher a StyleGAN2 ModulateConvBlock `L` runs on, and with which packed copy of its weight: the forward rule (`forward`) and the
data-gradient rule (`dgrad`) side by side, with the measurements behind them.  The switches (A/B measurements) are read once, at import."""
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


# ------------------------------------------------------------------ forward
def prepared(L, dtype):
    """-- derived weights, rebuilt only when the parameter changes: (packed copy for conv2d, per-(o,i) sum of squares)"""
    c = lookup(L._cache, ("w", dtype), L.weight)
    if c is None:
        mode = ops.PACK_UPFOLD if L.up else ops.PACK_FWD
        hin = L.res // 2 if L.up else L.res         # the low-resolution layers get fragment-ordered weights (conv_small)
        packed = ops.pack_conv_weight(L.weight, ops.pack_mode_for(L.weight, mode, hin, hin, dtype), dtype, L.wscale) \
            if L.ksize == 3 else None
        wsq = ops.weight_sumsq(L.weight, L.wscale) if L.demodulate else None
        c = store(L._cache, ("w", dtype), L.weight, (packed, wsq))
    return c


def _prepared_up(L, dtype):
    """[9 units][Cout][Cin] weights of the phase-form up kernel (ops.upconv_fir), or None when the layer shape is not
    covered by it (then the folded 3x3-per-phase form of conv2d(up=True) runs)."""
    # (input resolutions below 16: a single 16x16 t-pixel tile per sample would be mostly padding -- the folded form is faster)
    if not L.up or L.res < 32 or UP_FOLDED or not ops.upconv_supported(L.in_c, L.out_c, dtype):
        return None
    c = lookup(L._cache, ("wu", dtype), L.weight)
    return c if c is not None else store(L._cache, ("wu", dtype), L.weight, ops.pack_upconv_weight(L.weight, dtype, L.wscale))


def forward(L, x, s, d, noise, dt, rgb=None):
    """The modulated conv proper (:898-921) on NHWC activations: shared-weight form with s / d as prologue / epilogue scales.
    `rgb`: fused toRGB of the result (ops.conv2d), stride-1 layers only."""
    nw = L.noise_strength.detach().reshape(1) if noise is not None else None
    B, H, W, _ = x.shape
    wu = _prepared_up(L, dt)
    if wu is not None:
        assert rgb is None
        if (UP_PP and s is not None and d is not None and (noise is None or nw.numel() == 1)
                and ops.up_pp_supported(B, H, W, L.in_c, L.out_c, dt)):
            # MFMA-bound up layers (Cin >= 128): fused modulation (:858-875) folded into one weight image per sample, ping-pong
            # implicit GEMM with the FIR in registers (csrc/up_pp.hip)
            wimg = ops.pack_up_pp(wu, L.out_c, L.in_c, in_scale=s, out_scale=d, gain=L.gain)
            return ops.up_pp(x, wimg, L.out_c, bias=L.bias, bias_scale=L.bscale, noise=noise, noise_w=nw, act=L.act, gain=L.gain)
        return ops.upconv_fir(x, wu, L.out_c, in_scale=s, out_scale=d, bias=L.bias, bias_scale=L.bscale, noise=noise, noise_w=nw, act=L.act, gain=L.gain)
    if (rgb is None and not L.up and d is not None and s is not None and L.ksize == 3 and PP_GEN
            and ops.conv_pp_supported(B, H, W, L.in_c, L.out_c, dt)):
        # MFMA-bound layers (>= 128 channels at 64^2 .. 256^2): the reference's fused modulation (:858-875) - style, demodulation
        # and gain folded into one weight image per sample - feeding the ping-pong implicit GEMM (csrc/conv_pp.hip)
        wpp = ops.pack_conv_pp(L.weight, L.wscale, in_scale=s, out_scale=d, gain=L.gain)
        return ops.conv_pp(x, wpp, L.out_c, bias=L.bias, bias_scale=L.bscale, noise=noise, noise_w=nw, act=L.act, gain=L.gain)
    packed, _ = prepared(L, dt)
    return ops.conv2d(x, packed, L.out_c, 3, up=L.up, in_scale=s, out_scale=d, bias=L.bias, bias_scale=L.bscale, noise=noise, noise_w=nw, act=L.act, gain=L.gain, rgb=rgb)


# ------------------------------------------------------------------ data gradient
def _up_phase_form(L):
    """Up layers whose data gradient runs in phase form (FIR^T pass + 4-tap conv on the t grid, dge_fir_t2d / in_t2d: 16 tap-units
    per input pixel instead of the 36 of the folded space-to-depth form): the MFMA-bound ones, 32^2 .. 128^2 input (measured at
    batch 8, tools/perf_t2d.py, folded -> FIR pass + conv: 512->512 @32^2 221 -> 174 us, 256<-512 @64^2 310 -> 243, 128<-256 @128^2
    344 -> 313; at 256^2 / 512^2 the launch is bound by its epilogue and the extra pass loses: 430 -> 504, 951 -> 1223).  On
    conv2d the small grids stay on the folded form; in fused bf16 mode the 256 / 512-channel layers up to 32^2 take the phase form
    of the low-resolution kernel instead (_up_small_dgrad, checked first)."""
    return L.up and 32 <= L.res // 2 <= 128 and L.in_c >= 64 and L.in_c % 32 == 0 and L.out_c % 8 == 0 and T2D


def _dgrad_weight(L, dtype):
    hg = L.res // 2 if L.up else L.res          # grid the data-gradient conv runs on (space-to-depth grid for the up layers)
    if _up_phase_form(L):
        mode = ops.PACK_UPT2D_DGRAD
    else:
        mode = ops.pack_mode_for(L.weight, ops.PACK_UPFOLD_DGRAD if L.up else ops.PACK_DGRAD, hg, hg, dtype)
    c = lookup(L._cache, ("dg", dtype, mode), L.weight)
    return c if c is not None else store(L._cache, ("dg", dtype, mode), L.weight, ops.pack_conv_weight(L.weight, mode, dtype, L.wscale))


def _pp_dgrad(L, B, hg, dtype):
    """the data gradient of this layer runs on conv_pp (GEMM K = out channels, x 4 phases for the folded up layer; N = in channels)"""
    K = 4 * L.out_c if L.up else L.out_c
    return PP_DG and (not L.up or L.out_c % 32 == 0) and ops.conv_pp_supported(B, hg, hg, K, L.in_c, dtype)


def _dgrad_weight_pp(L, d, t2d=False):
    """data-gradient weight image of conv_pp.  Stride 1 / folded up layer: per sample, W'[b] = bf16(w * wscale * d[b, o]) (the up layer
    through its folded f32 rows, packed once per weight version); phase form: one shared 4-tap image, cached per weight version"""
    if not L.up:
        return ops.pack_conv_pp(L.weight, L.wscale, in_scale=d, dgrad=True)
    name = "dgpp_t2d" if t2d else "dgpp"
    c = lookup(L._cache, name, L.weight)
    if c is None:
        rows = ops.pack_conv_weight(L.weight, ops.PACK_UPT2D_DGRAD if t2d else ops.PACK_UPFOLD_DGRAD, ops.F32, L.wscale)
        c = store(L._cache, name, L.weight, ops.pack_conv_pp_rows(rows, L.in_c, t2d=True) if t2d else rows)
    return c if t2d else ops.pack_conv_pp_rows(c, L.in_c, in_scale=d, in_period=L.out_c)


def _up_stream_dgrad(L, B, dtype, fused):
    """the data gradient of this up layer runs on the streaming adjoint kernel (ops.up_dgrad_stream: 64 <- 32 channels, bf16; fused
    mode only - its sums leave by atomics)"""
    return UP_DG_STREAM and fused and L.up and L.ksize == 3 and ops.up_dgrad_stream_supported(B, L.res // 2, L.res // 2, L.in_c, L.out_c, dtype)


def _dgrad_weight_stream(L, dtype):
    c = lookup(L._cache, ("dgs", dtype), L.weight)
    return c if c is not None else store(L._cache, ("dgs", dtype), L.weight, ops.pack_up_dgrad_stream(L.weight, dtype, L.wscale))


def _up_small_dgrad(L, B, dtype, fused):
    """the data gradient of this up layer runs in phase form on the low-resolution kernel (ops.up_dgrad_small after ops.fir_t2d: 256 /
    512 channels on a grid <= 32^2, bf16; fused mode only - deterministic mode and f32 keep their launches)"""
    return UP_DG_SMALL and fused and L.up and L.ksize == 3 and ops.up_dgrad_small_supported(B, L.res // 2, L.res // 2, L.in_c, L.out_c, dtype)


def _dgrad_weight_small(L, dtype):
    c = lookup(L._cache, ("dgu", dtype), L.weight)
    return c if c is not None else store(L._cache, ("dgu", dtype), L.weight, ops.pack_up_dgrad_small(L.weight, dtype, L.wscale))


def dgrad_takes_prep(L, B=None, dtype=None):
    """True when the data-gradient launch of L may carry the tail backward of the layer below in its epilogue (`prep`)
    (the space-to-depth data gradient of a narrow up layer - layer 15: 64 -> 32 channels - loses more in its 64-wide conv_igemm tile
     than the separate pass costs: measured 890 vs 747 us; tools/perf_prep.py.  The streaming adjoint carries it: the stored
     activation of the layer below is in its registers for the dot products anyway.)"""
    if B is not None and L.up and _up_stream_dgrad(L, B, dtype, not ops.is_deterministic()):
        return True
    return _up_phase_form(L) or not (L.up and L.in_c < 128)


def dgrad(L, g_y, d_in, dt, fused, prep=None, **epilogue):
    """g_xprev [B,Hin,Win,in_c] of layer L from g_y; d_in: the demodulation factor still to be applied to g_y, or None.
    `prep` and `epilogue` (out_scale, addend, stats, dot_src) go to the launch as they are (ops.conv2d / ops.conv_pp)."""
    B, hg = g_y.shape[0], (L.res // 2 if L.up else L.res)
    if L.up and _up_stream_dgrad(L, B, dt, fused) and epilogue.get("dot_src") is not None and epilogue.get("stats") is not None \
            and set(epilogue) <= {"out_scale", "addend", "stats", "dot_src"}:
        # narrow up layer (64 <- 32): FIR^T, the 9-tap adjoint on the t grid and the epilogue in one streaming pass
        return ops.up_dgrad_stream(g_y, _dgrad_weight_stream(L, dt), d_in, epilogue.get("out_scale"), epilogue.get("addend"),
                                   epilogue.get("stats"), epilogue["dot_src"], prep=prep)
    if L.up and _up_small_dgrad(L, B, dt, fused) and set(epilogue) <= {"out_scale", "addend", "stats", "dot_src"}:
        # low-resolution up layers (512 <- 512 at 4^2 .. 32^2): FIR^T to the t grid, then the 9 non-zero units on the low-resolution kernel
        return ops.up_dgrad_small(ops.fir_t2d(g_y, d_in), _dgrad_weight_small(L, dt), epilogue.get("out_scale"), epilogue.get("addend"),
                                  epilogue.get("stats"), epilogue.get("dot_src"), prep=prep)
    t2d = _up_phase_form(L)
    if fused and d_in is not None and not t2d and _pp_dgrad(L, B, hg, dt):
        # MFMA-bound launches on the ping-pong kernel (csrc/conv_pp.hip): the demodulation factor is folded into a per-sample
        # weight image instead of scaling g_z in a prologue
        return ops.conv_pp(g_y, _dgrad_weight_pp(L, d_in), L.in_c, dgrad=True, in_s2d=L.up, add_scale=1.0, prep=prep, **epilogue)
    if t2d and fused and prep is not None and _pp_dgrad(L, B, hg, dt):
        # phase form on the ping-pong kernel: the same FIR^T pass, then the 4-tap conv with ONE shared weight image
        return ops.conv_pp(ops.fir_t2d(g_y, d_in), _dgrad_weight_pp(L, None, t2d=True), L.in_c, dgrad=True, in_t2d=True, add_scale=1.0, prep=prep, **epilogue)
    if t2d:      # phase form: FIR^T (times the demodulation factor) to the t grid, then the 4-tap conv
        return ops.conv2d(ops.fir_t2d(g_y, d_in), _dgrad_weight(L, dt), L.in_c, 3, in_t2d=True, add_scale=1.0, prep=prep, **epilogue)
    return ops.conv2d(g_y, _dgrad_weight(L, dt), L.in_c, 3, in_s2d=L.up, in_scale=d_in, add_scale=1.0, prep=prep, **epilogue)
