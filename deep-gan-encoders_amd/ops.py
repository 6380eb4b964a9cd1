"""Tensor-level wrappers over the C ABI (include/dge_hip.h).  PyTorch supplies device memory
and the stream; every computation happens in libdge_hip.so."""
import ctypes as C
import math

import torch

from ._lib import lib, check, ConvDesc, ConvPPDesc, DgeError, last_kernel

F32, BF16 = 0, 1
ACT_NONE, ACT_LRELU, ACT_RELU, LIN_RSQRT = 0, 1, 2, 3
PACK_FWD, PACK_UPFOLD, PACK_DGRAD, PACK_UPFOLD_DGRAD, PACK_SG1_UP, PACK_SG1_UP_DGRAD, PACK_UPT2D_DGRAD = 0, 1, 2, 3, 4, 5, 6
PACK_UPT2D_UNITS = 7  # the 9 non-zero (phase, offset) units of PACK_UPT2D_DGRAD, [9, Cin, Cout], in up_dgrad_small's walk order
PACK_FRAG = 0x100     # OR-ed into a pack mode: MFMA-fragment order for the low-resolution kernel (csrc/conv_small.hip)
import os as _os
import weakref as _weakref
KERNEL_LOG = None   # tests set this to a list: (kernel instantiation name, stream handle) per conv_pp / up_pp launch (which streams ran them)
PROFILE = None      # bench.py sets this to a list: (start_event, stop_event, algorithmic_flops, tag, algorithmic_bytes) per conv launch


class _ZeroArena:
    """Pre-zeroed float32 scratch for the many small accumulation targets of one training step
    (statistics slots, reduction outputs, weight-gradient buffers).  One memset per step replaces
    a fill launch per buffer.  Tensors handed out are views: they stay valid until the arena is
    re-armed by the next `zero_arena_begin()`."""

    def __init__(self):
        self.buf, self.off, self.high, self.active = None, 0, 0, False


_ARENA = _ZeroArena()


def zero_arena_begin(device, nbytes=512 << 20):
    a = _ARENA
    if a.buf is None or a.buf.device != torch.device(device) or a.buf.numel() * 4 < nbytes:
        a.buf = torch.zeros(nbytes // 4, dtype=torch.float32, device=device)
    else:
        a.buf[:a.high].zero_()
    a.off, a.high, a.active = 0, 0, True


def zero_arena_end():
    _ARENA.active = False


def zeros(shape, device):
    """float32 zeros; served from the step arena when one is armed, else a plain allocation."""
    a = _ARENA
    n = int(math.prod(shape))
    if a.active and a.buf.device == torch.device(device) and a.off + n <= a.buf.numel():
        t = a.buf[a.off:a.off + n].view(shape)
        a.off = (a.off + n + 63) & ~63
        a.high = max(a.high, a.off)
        return t
    return torch.zeros(shape, dtype=torch.float32, device=device)


class SlotStats:
    """Per-(b,c) statistics target [B,C,2] whose slot copies (dge_conv2d spreads its statistics atomics over up to 64 copies,
    same-address contention) are added by the CONSUMING kernel (stats_finalize / in_bwd_coef) instead of a dge_sum_slots launch."""
    __slots__ = ("B", "C", "device", "buf", "nslot")

    def __init__(self, B, C, device):
        self.B, self.C, self.device, self.buf, self.nslot = B, C, device, None, 1

    def alloc(self, nslot):
        self.nslot = nslot
        self.buf = zeros((nslot, self.B, self.C, 2), self.device)
        return self.buf

    def plain(self):
        """a [B,C,2] tensor for producers that do not use slots (fromrgb, blend)"""
        return self.alloc(1)[0]


def sum_slots(partial, out, accumulate=True):
    """out [...] (+)= the sum of partial [n, ...] over its leading axis (dge_sum_slots): the slot copies of a statistics target"""
    check(lib().dge_sum_slots(_p(partial), _p(out), partial.shape[0], out.numel(), 1 if accumulate else 0, _stream()), "dge_sum_slots")
    return out


def _sum_over_batch(partial, out=None):
    """partial [B, ...] per-sample sums -> [...] (dge_sum_slots); accumulates into `out` when given."""
    if out is not None:
        return sum_slots(partial, out)
    return sum_slots(partial, torch.empty(partial.shape[1:], dtype=torch.float32, device=partial.device), accumulate=False)


# ------------------------------------------------------------------ counter-based noise (dge_randn)
class _Noise:
    """State of the step's noise draws: `seed` (set by generators.set_seed next to torch / numpy), a draw counter that names the
    Philox subsequence of each tensor, and the data-parallel position (rank, world): a draw of per-sample rows [B, ...] is the
    rank's slice of the global-batch tensor [world*B, ...], so N ranks x B reproduce one process at batch N*B exactly."""

    def __init__(self):
        self.seed, self.counter, self.rank, self.world, self.seed_dev, self.graph_base = None, 0, 0, 1, None, 0


NOISE = _Noise()


def noise_seed(seed):
    NOISE.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    NOISE.counter = 0
    if NOISE.seed_dev is not None:
        # a fresh pageable host tensor per call: staged before copy_ returns, so the host may run replays ahead
        NOISE.seed_dev.copy_(torch.tensor([NOISE.seed - (1 << 64) if NOISE.seed >= (1 << 63) else NOISE.seed], dtype=torch.int64))


def noise_dp(rank, world):
    NOISE.rank, NOISE.world = int(rank), int(world)


def noise_graph_begin(device):
    """hipGraph mode: from now on the kernels read the seed from a device scalar that noise_seed() refreshes before each replay.
    The scalar is allocated once per device and kept: a captured graph holds its address, and a second capture in the process
    must not free it under the first graph."""
    if NOISE.seed_dev is None or NOISE.seed_dev.device != torch.empty(0, device=device).device:
        NOISE.seed_dev = torch.zeros(1, dtype=torch.int64, device=device)
    NOISE.graph_base = NOISE.seed or 0
    if NOISE.seed is not None:
        noise_seed(NOISE.seed)


def noise_graph_seed(iteration):
    """hipGraph mode, for loops that do not seed their iterations themselves: a new seed per iteration, counted from the seed that
    was in force at noise_graph_begin.  A function of the iteration number alone: an iteration that is recorded, not executed,
    leaves nothing to roll back."""
    noise_seed(NOISE.graph_base + iteration + 1)


def randn_rows(shapes, device):
    """Normal noise tensors of per-sample shapes [(B, ...), ...] in ONE launch (contiguous slices of one buffer).  Tensor k
    is draw number `counter + k`; its elements are those of rows [rank*B, (rank+1)*B) of the global [world*B, ...] tensor."""
    if NOISE.seed is None:
        noise_seed(torch.initial_seed())
    n = len(shapes)
    sizes = [int(math.prod(sh)) for sh in shapes]
    starts, off = [], 0
    for sz in sizes:
        starts.append(off)
        off += (sz + 3) & ~3                       # keep every tensor 16-byte aligned
    flat = torch.empty(max(off, 1), dtype=torch.float32, device=device)
    LL, ULL, UI = C.c_longlong * n, C.c_ulonglong * n, C.c_uint * n
    goff = [NOISE.rank * sz for sz in sizes]
    sub = [(NOISE.counter + k) & 0xFFFFFFFF for k in range(n)]
    NOISE.counter += n
    sd = C.c_void_p(NOISE.seed_dev.data_ptr()) if NOISE.seed_dev is not None else None
    check(lib().dge_randn(_p(flat), n, LL(*starts), LL(*sizes), ULL(*goff), UI(*sub), C.c_ulonglong(NOISE.seed), sd, _stream()),
          "dge_randn")
    return [flat[st:st + sz].view(sh) for st, sz, sh in zip(starts, sizes, shapes)]


def randn(shape, device):
    return randn_rows([tuple(shape)], device)[0]


def tdtype(dtype):
    return torch.bfloat16 if dtype == BF16 else torch.float32


def dtype_of(t):
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float32:
        return F32
    raise DgeError(f"unsupported activation dtype {t.dtype}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """The current stream of the current device as a hipStream_t.  torch.cuda.current_stream() builds a Stream object through
    several Python layers (~4 us); with ~850 launches per step that was a fifth of the host time at batch 2, so the raw
    handle is fetched directly when this torch exposes it."""
    if _raw_stream is not None and _raw_device is not None:
        return C.c_void_p(_raw_stream(_raw_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise DgeError("tensor is not on the GPU: the HIP path has no CPU fallback")
    if not t.is_contiguous():
        raise DgeError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def _f32(t):
    if t is not None and t.dtype != torch.float32:
        raise DgeError(f"expected float32, got {t.dtype}")
    return _p(t)


def packed_n(n):
    return lib().dge_packed_n(int(n))


def small_conv(H, W, kdim, nvalid, ksize=3, in_s2d=False, in_up2=False, dtype=BF16):
    """True when dge_conv2d runs a launch of this shape (input grid H x W, packed K = kdim, N = nvalid before padding) on the
    low-resolution kernel: its weights must then be packed with `mode | PACK_FRAG`."""
    return bool(lib().dge_conv_small_supported(int(H), int(W), int(kdim), packed_n(nvalid), int(ksize), int(bool(in_s2d)),
                                               int(bool(in_up2)), int(dtype)))


def _pack_io(w, mode):
    """(cout, cin) of the conv whose parameter w is (ConvTranspose2d parameter layout [Cin, Cout, k, k] for the SG1 up modes)"""
    return (w.shape[1], w.shape[0]) if (mode & 0xff) in (PACK_SG1_UP, PACK_SG1_UP_DGRAD) else (w.shape[0], w.shape[1])


def pack_dims(w, mode):
    """(nvalid, kdim) of the packed copy of w [Cout,Cin,k,k] in pack mode `mode`"""
    cout, cin = _pack_io(w, mode)
    mode &= 0xff
    nvalid = 4 * cout if mode in (PACK_UPFOLD, PACK_SG1_UP) else (cin if mode in (PACK_DGRAD, PACK_UPFOLD_DGRAD, PACK_SG1_UP_DGRAD, PACK_UPT2D_DGRAD, PACK_UPT2D_UNITS) else cout)
    kdim = cout if mode in (PACK_DGRAD, PACK_UPT2D_UNITS) else (4 * cout if mode in (PACK_UPFOLD_DGRAD, PACK_SG1_UP_DGRAD, PACK_UPT2D_DGRAD) else cin)
    return nvalid, kdim


def pack_mode_for(w, mode, H, W, dtype):
    """`mode`, with PACK_FRAG added when the conv that reads this copy at input resolution H x W runs on the low-resolution kernel"""
    nvalid, kdim = pack_dims(w, mode)
    in_s2d = (mode & 0xff) in (PACK_UPFOLD_DGRAD, PACK_SG1_UP_DGRAD)
    return mode | PACK_FRAG if small_conv(H, W, kdim, nvalid, w.shape[-1], in_s2d, False, dtype) else mode


def pack_conv_weight(w, mode=PACK_FWD, dtype=BF16, scale=1.0):
    """w: [Cout,Cin,k,k] f32 (reference layout) -> packed [k*k, Npad, K] tensor of `dtype`; with `mode | PACK_FRAG` the same values in
    MFMA-fragment order (the tensor carries `_dge_frag = True`, which conv2d hands on as dge_conv_desc.w_layout)."""
    (cout, cin), k = _pack_io(w, mode), w.shape[2]
    nvalid, kdim = pack_dims(w, mode)
    out = torch.empty((k * k, packed_n(nvalid), kdim), dtype=tdtype(dtype), device=w.device)
    check(lib().dge_pack_conv_weight(_f32(w.detach().contiguous()), _p(out), cout, cin, k, mode, dtype, float(scale),
                                     _stream()), "dge_pack_conv_weight")
    if mode & PACK_FRAG:
        out._dge_frag = True
    return out


def set_deterministic(on=True):
    """Deterministic mode of the library (the reference pins torch.backends.cudnn.deterministic = True, training_utils.py:51):
    every reduction that ends in same-address f32 atomics - conv statistics, weight-gradient flush, the per-channel sums of
    the streaming backward kernels, loss sums - goes through per-contributor slots and an ordered sum by the last contributor
    instead (csrc/common.h).  Run to run the results are then bit-identical.  Synchronises the device."""
    check(lib().dge_set_deterministic(1 if on else 0), "dge_set_deterministic")


def is_deterministic():
    return bool(lib().dge_get_deterministic())


def pack_conv_weights_multi(entries, scratch=None):
    """entries: [(w [Cout,Cin,k,k] f32, mode, dtype, scale, out)] with `out` the tensors pack_conv_weight returned for the same
    arguments: refreshes all of them in ONE launch.  Returns the device scratch (pass it back to reuse it)."""
    import struct
    n = len(entries)
    if n == 0:
        return scratch
    rows = []
    for (w, mode, dtype, scale, out) in entries:
        (cout, cin), k = _pack_io(w, mode), w.shape[2]
        if not (w.is_cuda and w.is_contiguous() and w.dtype == torch.float32):
            raise DgeError("pack_conv_weights_multi: weights must be contiguous f32 device tensors")
        rows += [w.data_ptr(), out.data_ptr(), cout | (cin << 32), k | (mode << 32), dtype,
                 struct.unpack("<I", struct.pack("<f", float(scale)))[0], 0, 0]
    tab = (C.c_longlong * (8 * n))(*rows)
    need = n * lib().dge_pack_desc_bytes()
    key = tuple(rows)
    if scratch is None or scratch[0].numel() < need:
        scratch = [torch.empty(max(need, 4096), dtype=torch.uint8, device=entries[0][0].device), None]
    upload = 0 if scratch[1] == key else 1          # same table as the last call: the descriptors are already on the device
    check(lib().dge_pack_conv_weights_multi(tab, _p(scratch[0]), n, upload, _stream()), "dge_pack_conv_weights_multi")
    scratch[1] = key
    return scratch


def weight_sumsq(w, scale=1.0):
    cout, cin, k, _ = w.shape
    out = torch.empty((cout, cin), dtype=torch.float32, device=w.device)
    check(lib().dge_weight_sumsq(_f32(w.detach().contiguous()), _p(out), cout, cin, k, float(scale), _stream()),
          "dge_weight_sumsq")
    return out


def linear(x, w, bias=None, wscale=1.0, bscale=1.0, add=0.0, act=ACT_NONE, gain=1.0, square_input=False, out=None):
    """x: [B, I] f32 view with unit inner stride (row stride arbitrary); w: [O, I]."""
    B, I = x.shape
    O = w.shape[0]
    if x.stride(1) != 1:
        raise DgeError("linear: inner stride must be 1")
    if out is None:
        out = torch.empty((B, O), dtype=torch.float32, device=x.device)
    if not x.is_cuda:
        raise DgeError("tensor is not on the GPU: the HIP path has no CPU fallback")
    check(lib().dge_linear(C.c_void_p(x.data_ptr()), x.stride(0), _f32(w), _f32(bias), C.c_void_p(out.data_ptr()),
                           out.stride(0), B, I, O, float(wscale), float(bscale), float(add), act, float(gain),
                           1 if square_input else 0, _stream()), "dge_linear")
    _log_dense("dge_linear")
    return out


def _dense_layers(layers):
    from ._lib import DenseLayer
    arr = (DenseLayer * len(layers))()
    for e, L in zip(arr, layers):
        e.w, e.bias = _p(L.weight.detach()), _p(L.bias.detach())
        e.O, e.I = L.weight.shape
        e.wscale, e.bscale, e.add, e.act, e.gain = float(L.wscale), float(L.bscale), float(L.additional_bias), int(L.act), float(L.gain)
    return arr


def mapping_bwd_work_bytes(B):
    """Bytes of the workspace dge_mapping_bwd_wide needs for B samples."""
    n = lib().dge_mapping_bwd_wide_work_bytes(int(B))
    if n < 0:
        check(n, "dge_mapping_bwd_wide_work_bytes")
    return n


def mapping_bwd(z, layers, g, coefs=None, acts=None, pixelnorm=True, eps=1e-8, wide=False, work=None, out=None):
    """Data gradient of w+ = lerp(avg, broadcast_L(chain(z)), coefs) in one launch (dge_mapping_bwd): z [B, I] f32, g = dL/dw+
    [B, L, O] f32, coefs [L] f32 or None (plain broadcast), acts: the forward's layer outputs ([B, O_l] each; the leaky-relu masks
    are read off them) or None (the launch recomputes the forward) -> dz [B, I].  The same bits every run.
    wide=True: dge_mapping_bwd_wide, one chip-wide launch per layer and a tail (acts required; `work`: a uint8 workspace of
    mapping_bwd_work_bytes(B) bytes, allocated when None); row b has the bits of the row run alone.  `out`: dz goes into this
    [B, I] f32 tensor (unit inner stride, any row stride)."""
    B, L = g.shape[0], g.shape[1]
    if not z.is_cuda or z.stride(1) != 1:
        raise DgeError("mapping_bwd: z must be a CUDA tensor with unit inner stride")
    if z.shape[1] != layers[0].weight.shape[1] or z.shape[0] != B:
        raise DgeError(f"mapping_bwd: z {tuple(z.shape)} does not match B = {B}, first layer width {layers[0].weight.shape[1]}")
    g = g.float().contiguous()
    if g.shape[2] != layers[-1].weight.shape[0]:
        raise DgeError(f"mapping_bwd: gradient width {g.shape[2]} != last layer width {layers[-1].weight.shape[0]}")
    if coefs is not None and coefs.numel() != L:
        raise DgeError(f"mapping_bwd: {coefs.numel()} coefficients for {L} rows")
    arr = arr_p = None
    if acts is not None:
        if len(acts) != len(layers) or any(tuple(a.shape) != (B, Ly.weight.shape[0]) for a, Ly in zip(acts, layers)):
            raise DgeError("mapping_bwd: acts must hold one [B, O_l] output per layer")
        arr = (C.c_void_p * len(acts))(*[_f32(a).value for a in acts])
        arr_p = C.cast(arr, C.c_void_p)
    if out is None:
        dz = torch.empty((B, z.shape[1]), dtype=torch.float32, device=z.device)
    else:
        dz = out
        if not dz.is_cuda or dz.dtype != torch.float32 or tuple(dz.shape) != (B, z.shape[1]) or dz.stride(1) != 1:
            raise DgeError("mapping_bwd: out must be a [B, I] f32 CUDA tensor with unit inner stride")
    coefs_p = _f32(None if coefs is None else coefs.contiguous())
    if wide:
        if acts is None:
            raise DgeError("mapping_bwd: wide=True needs the saved layer outputs (acts); the recompute form is the one-launch kernel's")
        need = mapping_bwd_work_bytes(B)
        if work is None:
            work = torch.empty(need, dtype=torch.uint8, device=z.device)
        elif not work.is_cuda or work.dtype != torch.uint8 or not work.is_contiguous() or work.numel() < need:
            raise DgeError(f"mapping_bwd: work must be a contiguous uint8 CUDA tensor of at least {need} bytes")
        if z.dtype != torch.float32:
            raise DgeError(f"expected float32, got {z.dtype}")
        # (z and dz by address: rows of any stride)
        check(lib().dge_mapping_bwd_wide(C.c_void_p(z.data_ptr()), z.stride(0), _dense_layers(layers), len(layers), arr_p, _p(g), L, coefs_p,
                                         C.c_void_p(dz.data_ptr()), dz.stride(0), B, 1 if pixelnorm else 0, float(eps), _p(work), work.numel(), _stream()),
              "dge_mapping_bwd_wide")
        _log_dense("dge_mapping_bwd_wide")
        return dz
    check(lib().dge_mapping_bwd(_f32(z), z.stride(0), _dense_layers(layers), len(layers), arr_p, _p(g), L,
                                coefs_p, _p(dz), dz.stride(0), B, 1 if pixelnorm else 0,
                                float(eps), _stream()), "dge_mapping_bwd")
    return dz


def dense_chain(x, layers, pixelnorm=False, eps=1e-8):
    """x [B, I] f32 through a chain of up to 8 dense layers in one launch (dge_dense_chain; bit-identical to the per-layer linear()
    calls).  layers: objects with weight [O, I], bias, wscale, bscale, additional_bias, act, gain (DenseBlock)."""
    B = x.shape[0]
    arr = _dense_layers(layers)
    y = torch.empty((B, layers[-1].weight.shape[0]), dtype=torch.float32, device=x.device)
    if not x.is_cuda or x.stride(1) != 1:
        raise DgeError("dense_chain: x must be a CUDA tensor with unit inner stride")
    check(lib().dge_dense_chain(_f32(x), x.stride(0), arr, len(layers), _p(y), y.stride(0), B, 1 if pixelnorm else 0, float(eps), _stream()),
          "dge_dense_chain")
    return y


def pixelnorm(x, eps=1e-8):
    y = torch.empty_like(x)
    check(lib().dge_pixelnorm(_f32(x), _p(y), x.shape[0], x.shape[1], eps, _stream()), "dge_pixelnorm")
    return y


def truncation(w, w_avg, num_layers, psi, layers):
    w_is_wp = (w.ndim == 3)
    B, D = w.shape[0], w.shape[-1]
    wp = torch.empty((B, num_layers, D), dtype=torch.float32, device=w.device)
    check(lib().dge_truncation(_f32(w.contiguous()), _f32(w_avg), _p(wp), B, num_layers, D, float(psi), int(layers),
                               1 if w_is_wp else 0, _stream()), "dge_truncation")
    return wp


def log_kernel():
    """KERNEL_LOG hook: records (name of the kernel the library launched last, current stream handle)"""
    if KERNEL_LOG is not None:
        KERNEL_LOG.append((last_kernel(), _stream()))


def _log_dense(name):
    """KERNEL_LOG entry of a dense-layer entry point (they select no kernel instantiation: the entry point's name)"""
    if KERNEL_LOG is not None:
        KERNEL_LOG.append((name, _stream()))


def _launch(fn, args, name, macs, tag, tensors, wbytes=0, log=False):
    """The one launch path of the conv family (dge_conv2d, dge_conv_pp, dge_up_pp, dge_upconv_fir): check(fn(*args)), timed by an
    event pair when PROFILE is a list - the entry is (start, stop, algorithmic flops = 2 * macs, tag, algorithmic bytes = every tensor
    of `tensors` crossing HBM once, + wbytes for weights counted by formula) - and named in KERNEL_LOG when `log`."""
    if PROFILE is None:
        check(fn(*args), name)
    else:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(fn(*args), name)
        e1.record()
        PROFILE.append((e0, e1, 2.0 * macs, tag, sum(t.numel() * t.element_size() for t in tensors if t is not None) + wbytes))
    if log and KERNEL_LOG is not None:
        log_kernel()


def _stats_slots(B, H, W, tile_w):
    """Copies that the statistics atomics of a launch on an H x W grid are spread over (same-address contention): one per 16 tiles
    of 16 x tile_w pixels - the kernel's tile: 16 wide for dge_conv2d, 32 for dge_conv_pp - and 64 at the most."""
    return max(1, min(64, ((H + 15) // 16) * ((W + tile_w - 1) // tile_w) * B // 16))


def _mask_as_dot_src(name, relu_mask, dot_src, prep):
    """the stored activation of `relu_mask` reaches the kernel in the dot_src operand, so it excludes dot_src and prep"""
    if relu_mask is not None and (dot_src is not None or prep is not None):
        raise DgeError(f"{name}: relu_mask excludes dot_src / prep")
    return dot_src if relu_mask is None else relu_mask


def _stats_target(stats, B, H, W, tile_w, device, spread_plain=True):
    """The statistics-slot protocol of a launch on an H x W grid -> (tensor the kernel adds into, its slot count, finish).  `stats`:
    None; a SlotStats, allocated here with the launch's slot count (the consuming kernel adds the copies); or a plain zeroed
    [B,C,2] tensor - the launch then spreads its atomics over partial copies of its own, and `finish()`, called after the launch,
    adds them into it (dge_sum_slots).  spread_plain=False: a plain tensor takes the atomics itself, as one slot."""
    nslot = _stats_slots(B, H, W, tile_w)
    if isinstance(stats, SlotStats):
        return stats.alloc(nslot), nslot, None
    if stats is None or nslot == 1 or not spread_plain:
        return stats, 1, None
    partial = zeros((nslot,) + tuple(stats.shape), device)
    return partial, nslot, lambda: sum_slots(partial, stats)


def _prep_values(prep, nslot):
    """the `prep` dict of the data-gradient launches -> (gain, noise, noise strength, batch of the noise, its statistics slots)"""
    pn = prep.get("noise")
    return float(prep["gain"]), pn, prep.get("ns") if pn is not None else None, 1 if pn is None else pn.shape[0], prep["stats"].alloc(nslot)


def _set_prep(d, prep, nslot):
    """the `prep` dict of conv2d / conv_pp -> the prep_* fields that dge_conv_desc and dge_conv_pp_desc share"""
    gain, pn, ns, nb, st = _prep_values(prep, nslot)
    d.prep, d.prep_gain, d.prep_noise, d.prep_ns, d.prep_noise_batch, d.prep_stats = 1, gain, _f32(pn), _f32(ns), nb, _f32(st)


def _weight_images(in_scale, out_scale):
    """number of weight images a pack_* call writes: one shared copy, or the batch of the per-sample scales (the last one given)"""
    t = in_scale if out_scale is None else out_scale
    return 1 if t is None else t.shape[0]


class _PrefetchChain:
    """L2 warm-up hint for the low-resolution kernel: the launch warms the weights of the low-resolution launch that followed it
    the LAST time it ran (a step repeats its launch sequence; packed copies keep their addresses) - dge_conv_desc.prefetch_w
    The chain is keyed by (stream, address): launches of different streams (the three loss windows) do not follow each other.
    An entry holds a WEAK reference to the packed tensor it points at: a re-allocated copy (load_state_dict, a new model) makes
    the entry stale and it is dropped instead of warming freed memory; the table is bounded."""

    def __init__(self, on=True):
        self.on, self.prev, self.next = on, {}, {}       # prev: stream -> address; next: (stream, address) -> (next address, ntot, cin, weakref)

    def link(self, stream, w_packed):
        """Records that `w_packed` follows the stream's previous launch; returns (ptr, ntot, cin) of what followed it last time, or None."""
        if not self.on:
            return None
        key = w_packed.data_ptr()
        prev = self.prev.get(stream)
        if prev is not None and prev != key:
            if len(self.next) > 512:
                self.next.clear()
            self.next[(stream, prev)] = (key, w_packed.shape[1], w_packed.shape[2], _weakref.ref(w_packed))
        self.prev[stream] = key
        nxt = self.next.get((stream, key))
        if nxt is None:
            return None
        t = nxt[3]()
        if t is None or t.data_ptr() != nxt[0]:
            del self.next[(stream, key)]
            return None
        return nxt[:3]


_PREFETCH = _PrefetchChain(on=not _os.environ.get("DGE_NO_PREFETCH"))


def conv2d(x, w_packed, cout, ksize=3, up=False, in_scale=None, in_shift=None, out_scale=None, bias=None,
           bias_scale=1.0, noise=None, noise_w=None, act=ACT_NONE, gain=1.0, addend=None, add_scale=1.0, stats=None,
           out=None, in_s2d=False, dot_src=None, in_up2=False, in_relu=False, prep=None, relu_mask=None, in_t2d=False, rgb=None, pool_out=False, pool_mask=False,
           in_bwd=None):
    """x: [B,H,W,Cin] NHWC (bf16 or f32).  Returns y [B,OH,OW,cout].
    `prep`: dict(gain, noise [1|B,OH,OW] or None, ns (device scalar) or None, stats=SlotStats(B, cout)) - the fused tail backward of
    the layer that produced `dot_src` (dge_conv_desc.prep): y is then g_z and prep['stats'] receives (sum g_z*(z - ns*noise), sum g_z).
    `relu_mask`: stored activation a = relu(pre) of the layer below: the result is multiplied by [a > 0] (dge_conv_desc.mask_relu).
    `rgb`: dict(w [3,cout] f32, style [B,cout], bias [3], wscale, out [B,3,H,W] f32, skip_y=False) - the toRGB of the result written
    by the same launch (dge_conv_desc.rgb_*, where conv_rgb_supported() says so); with skip_y the activation itself is not stored
    and None is returned.
    `in_bwd`: dict(coef [B,cout,3], noise [B,H,W] or None, red=SlotStats(B, cout)) - the instance-norm + activation backward of the
    layer input dot_src in the epilogue (dge_conv_desc.in_bwd_coef, where conv_in_bwd_supported() says so): y is g_pre, red receives
    (sum g_pre, sum g_pre*noise).
    `pool_out`: the launch stores the 2x2 average pool of its result, [B,OH/2,OW/2,cout] (dge_conv_desc.pool_out, where
    conv_pool_supported() says so); with pool_mask the signs of the full-resolution values come back too: returns (y, mask)."""
    B, H, W, Cin = x.shape
    if in_s2d:            # x is the fine grid [B,2H,2W,C]; logical input is [B,H,W,4C]
        H, W, Cin = H // 2, W // 2, Cin * 4
    if in_up2:            # x is the coarse grid; the conv runs on its nearest x2 upsample
        H, W = 2 * H, 2 * W
    if in_t2d:            # x is fir_t2d output [B,H+1,W+1,4C]; the conv runs on the H x W grid (phase-form adjoint of the up layer)
        H, W = H - 1, W - 1
    dt = dtype_of(x)
    OH, OW = (2 * H, 2 * W) if up else (H, W)
    mask = None
    if pool_out:
        if out is not None or up:
            raise DgeError("conv2d: pool_out allocates its own result and excludes up")
        out = torch.empty((B, OH // 2, OW // 2, cout), dtype=x.dtype, device=x.device)
        if pool_mask:
            mask = torch.empty((B, (OH // 2) * (OW // 2), cout // 8), dtype=torch.int32, device=x.device)
    if out is None:
        out = torch.empty((B, OH, OW, cout), dtype=x.dtype, device=x.device)
    d = ConvDesc()
    d.pool_out, d.pool_mask = 1 if pool_out else 0, _p(mask)
    dot_src = _mask_as_dot_src("conv2d", relu_mask, dot_src, prep)
    d.mask_relu = 0 if relu_mask is None else 1
    d.in_t2d = 1 if in_t2d else 0
    d.x, d.w_packed, d.y, d.addend, d.dot_src = _p(x), _p(w_packed), _p(out), _p(addend), _p(dot_src)
    d.in_scale, d.in_shift, d.out_scale = _f32(in_scale), _f32(in_shift), _f32(out_scale)
    # statistics atomics of large grids are spread over several copies (same-address contention), then combined
    st, nslot, finish = _stats_target(stats, B, H, W, 16, x.device)
    d.bias, d.noise, d.noise_w, d.stats = _f32(bias), _f32(noise), _f32(noise_w), _f32(st)
    d.stats_slots = nslot
    d.B, d.H, d.W, d.Cin, d.Cout = B, H, W, Cin, cout
    d.ksize, d.up, d.in_s2d, d.in_up2 = ksize, 1 if up else 0, 1 if in_s2d else 0, 1 if in_up2 else 0
    d.in_relu = 1 if in_relu else 0
    d.w_layout = 1 if getattr(w_packed, "_dge_frag", False) else 0
    if d.w_layout:
        nxt = _PREFETCH.link(_stream().value or 0, w_packed)
        if nxt is not None:
            d.prefetch_w, d.prefetch_ntot, d.prefetch_cin = C.c_void_p(nxt[0]), int(nxt[1]), int(nxt[2])
    if prep is not None:
        if stats is None or dot_src is None:
            raise DgeError("conv2d: prep needs stats and dot_src")
        _set_prep(d, prep, nslot)
    if in_bwd is not None:
        if dot_src is None or stats is not None or prep is not None:
            raise DgeError("conv2d: in_bwd needs dot_src and excludes stats / prep")
        d.stats_slots = _stats_slots(B, H, W, 16)
        pn = in_bwd.get("noise")
        d.in_bwd_coef = _f32(in_bwd["coef"])
        d.prep_noise, d.prep_noise_batch = _f32(pn), 1 if pn is None else pn.shape[0]
        if in_bwd.get("fr") is not None:          # FromRGB reduction flavour: nothing is stored, fr = SlotStats-like holder of [slots,B,cout,4]
            d.fr_img4, d.in_bwd_extra, d.in_bwd_extra_scale = _f32(in_bwd["img4"]), _p(in_bwd.get("extra")), float(in_bwd.get("extra_scale", 1.0))
            in_bwd["fr"].buf = zeros((d.stats_slots, B, cout, 4), x.device)
            d.fr_out = _f32(in_bwd["fr"].buf)
        elif in_bwd.get("red") is not None:
            d.prep_stats = _f32(in_bwd["red"].alloc(d.stats_slots))
        else:                                     # block-input form: no activation / reductions, pooled skip gradient added
            d.prep_noise = None
            d.in_bwd_extra, d.in_bwd_extra_scale = _p(in_bwd.get("extra")), float(in_bwd.get("extra_scale", 1.0))
    if rgb is not None:
        d.rgb_w, d.rgb_style, d.rgb_bias, d.rgb_out = _f32(rgb["w"]), _f32(rgb["style"]), _f32(rgb["bias"]), _f32(rgb["out"])
        d.rgb_wscale, d.rgb_skip_y = float(rgb["wscale"]), 1 if rgb.get("skip_y") else 0
    d.noise_batch = 1 if noise is None else noise.shape[0]
    d.noise_w_per_channel = 0 if (noise_w is None or noise_w.numel() == 1) else 1
    d.act, d.bias_scale, d.gain, d.add_scale, d.dtype = act, bias_scale, gain, add_scale, dt
    if w_packed.dtype != x.dtype:
        raise DgeError("conv2d: packed weight dtype differs from activation dtype")
    # algorithmic work: a folded up layer / its adjoint count as the 3x3 transposed conv they replace
    # (9*Cin*Cout MACs per INPUT pixel), everything else k*k*Cin*Cout per output pixel
    taps_cin = 9.0 * Cin if up else 9.0 * (Cin // 4) if (in_s2d or in_t2d) else float(ksize * ksize) * Cin
    # algorithmic bytes: every operand tensor crosses HBM once (input, output, optional addend / dot_src, packed weights)
    skip_y = rgb is not None and rgb.get("skip_y")
    _launch(lib().dge_conv2d, (C.byref(d), _stream()), "dge_conv2d", taps_cin * cout * H * W * B, (B, H, W, Cin, cout, ksize, up, in_s2d),
            (x, None if skip_y else out, addend, dot_src, w_packed, rgb["out"] if rgb is not None else None))
    if finish is not None:
        finish()
    if skip_y:
        return None
    if pool_out and pool_mask:
        return out, mask
    return out


def conv_in_bwd_supported(B, H, W, cin, cout, dtype):
    """True when a 3x3 data-gradient launch cin -> cout of this shape may carry the instance-norm backward epilogue (conv2d(in_bwd=...))"""
    return bool(lib().dge_conv_in_bwd_supported(int(B), int(H), int(W), int(cin), int(cout), 3, int(dtype)))


def conv_in_bwd_x_supported(B, H, W, cin, cout, dtype):
    return bool(lib().dge_conv_in_bwd_x_supported(int(B), int(H), int(W), int(cin), int(cout), 3, int(dtype)))


def conv_in_bwd_fromrgb_supported(B, H, W, cin, cout, dtype):
    return bool(lib().dge_conv_in_bwd_fromrgb_supported(int(B), int(H), int(W), int(cin), int(cout), 3, int(dtype)))


def up_pp_supported(B, H, W, cin, cout, dtype):
    """True when an up layer of this shape runs on the ping-pong kernel of csrc/up_pp.hip (Cin >= 128; H, W = the INPUT grid)"""
    return bool(lib().dge_up_pp_supported(int(B), int(H), int(W), int(cin), int(cout), int(dtype)))


def pack_up_pp(w_units, cout, cin, in_scale=None, out_scale=None, gain=1.0, out=None):
    """Weight image of up_pp from pack_upconv_weight's bf16 [9, Cout, Cin] units: one shared copy, or - with in_scale [B, Cin] /
    out_scale [B, Cout] - B copies with style, demodulation and gain folded in (stylegan2_generator.py:858-875).  [nb, 9*Cin*Cout] bf16."""
    if w_units.dtype != torch.bfloat16:
        raise DgeError("pack_up_pp: expects the bf16 units of pack_upconv_weight")
    nb = _weight_images(in_scale, out_scale)
    if out is None:
        out = torch.empty((nb, 9 * cin * cout), dtype=torch.bfloat16, device=w_units.device)
    check(lib().dge_pack_up_pp(_p(w_units), _p(out), int(cout), int(cin), _f32(in_scale), _f32(out_scale), float(gain), nb, _stream()),
          "dge_pack_up_pp")
    return out


def up_pp(x, w_img, cout, bias=None, bias_scale=1.0, noise=None, noise_w=None, act=ACT_NONE, gain=1.0):
    """x [B,H,W,Cin] bf16 -> y [B,2H,2W,cout]: conv_transpose2d(stride 2) + 4x4 FIR + noise / bias / activation (dge_up_pp) with the
    per-sample weight image of pack_up_pp (style, demodulation and gain folded in)."""
    B, H, W, Cin = x.shape
    if x.dtype != torch.bfloat16 or not x.is_cuda:
        raise DgeError("up_pp: bf16 CUDA activations only (the HIP path has no CPU fallback)")
    y = torch.empty((B, 2 * H, 2 * W, cout), dtype=x.dtype, device=x.device)
    nbs = 0 if (noise is None or noise.shape[0] == 1) else 4 * H * W
    if noise_w is not None and noise_w.numel() != 1:
        raise DgeError("up_pp: one noise strength per layer (stylegan2_generator.py:911-916)")
    wbs = 0 if w_img.shape[0] == 1 else w_img.stride(0)

    _launch(lib().dge_up_pp, (_p(x), _p(w_img), int(wbs), _p(y), _f32(noise), nbs, _f32(noise_w), _f32(bias), float(bias_scale),
                              float(gain), int(act), B, H, W, Cin, int(cout), _stream()), "dge_up_pp",
            9.0 * Cin * cout * H * W * B, (B, H, W, Cin, cout, 3, "upfir", False), (x, y), wbytes=18 * Cin * cout * B, log=True)
    return y


def conv_pp_supported(B, H, W, cin, cout, dtype):
    """True when a 3x3 stride-1 launch of this shape runs on the ping-pong implicit GEMM (csrc/conv_pp.hip: C >= 128 at 64^2 .. 256^2)"""
    return bool(lib().dge_conv_pp_supported(int(B), int(H), int(W), int(cin), int(cout), int(dtype)))


def pack_conv_pp(w, wscale=1.0, in_scale=None, out_scale=None, gain=1.0, dgrad=False, out=None):
    """LDS image of w [Cout,Cin,3,3] f32 for conv_pp: one shared copy, or - with in_scale [B,K] / out_scale [B,N] - B per-sample copies with
    style, demodulation and gain folded in (the reference's fused modulation, stylegan2_generator.py:858-875).  dgrad: the copy the
    data gradient reads ((n, k) = (in, out) channel, taps flipped).  Returns a [nb, 9*N*K] bf16 tensor."""
    cout, cin = w.shape[0], w.shape[1]
    N, K = (cin, cout) if dgrad else (cout, cin)
    nb = _weight_images(in_scale, out_scale)
    if out is None:
        out = torch.empty((nb, 9 * N * K), dtype=torch.bfloat16, device=w.device)
    check(lib().dge_pack_conv_pp(_f32(w.detach().contiguous()), _p(out), N, K, float(wscale), _f32(in_scale), _f32(out_scale), float(gain),
                                 nb, 1 if dgrad else 0, _stream()), "dge_pack_conv_pp")
    return out


def pack_conv_pp_rows(w_rows, N, in_scale=None, in_period=None, out_scale=None, gain=1.0, out=None, t2d=False):
    """The conv_pp weight image from an f32 pack_conv_weight copy w_rows [9, Npad, K] (rows 0 .. N-1 are used): the data-gradient
    layouts of the up layers.  in_scale [B, in_period] repeats along K (space-to-depth: the four phases of a channel)."""
    if w_rows.dtype != torch.float32 or w_rows.ndim != 3 or w_rows.shape[0] != 9:
        raise DgeError("pack_conv_pp_rows: expects an f32 [9, Npad, K] packed weight")
    K = w_rows.shape[2]
    nb = _weight_images(in_scale, out_scale)
    if out is None:
        out = torch.empty((nb, (4 if t2d else 9) * N * K), dtype=torch.bfloat16, device=w_rows.device)
    per = K if in_period is None else int(in_period)
    check(lib().dge_pack_conv_pp_rows(_f32(w_rows), int(w_rows.shape[1]), _p(out), int(N), int(K), _f32(in_scale), per, _f32(out_scale), float(gain),
                                      nb, 1 if t2d else 0, _stream()), "dge_pack_conv_pp_rows")
    return out


def conv_pp(x, w_pp, cout, out_scale=None, bias=None, bias_scale=1.0, noise=None, noise_w=None, act=ACT_NONE, gain=1.0, out=None,
            dgrad=False, in_s2d=False, dot_src=None, addend=None, add_scale=1.0, stats=None, prep=None, relu_mask=None, in_t2d=False):
    """x [B,H,W,Cin] bf16 -> y [B,H,W,cout]: 3x3 stride-1 conv with the weights of pack_conv_pp (w_pp.shape[0] = 1: shared, = B: per sample).
    dgrad: the data-gradient form (dge_conv_pp_desc.dgrad) with conv2d()'s menu: out_scale applied after the statistics
    stats (SlotStats) += (sum a*dot_src, sum a), addend, prep = dict(gain, noise, ns, stats=SlotStats), relu_mask; in_s2d: x is the fine
    grid [B,2H,2W,Cin/4]."""
    B, H, W, Cin = x.shape
    if in_s2d:
        H, W, Cin = H // 2, W // 2, Cin * 4
    if in_t2d:            # x is fir_t2d's [B,H+1,W+1,4C]: the conv runs on the H x W grid with the 4 taps of the phase form
        H, W = H - 1, W - 1
    if out is None:
        out = torch.empty((B, H, W, cout), dtype=x.dtype, device=x.device)
    if w_pp.shape[0] not in (1, B) or w_pp.shape[1] != (4 if in_t2d else 9) * Cin * cout or w_pp.dtype != torch.bfloat16:
        raise DgeError("conv_pp: weight image does not match the launch")
    d = ConvPPDesc()
    d.x, d.w_pp, d.y = _p(x), _p(w_pp), _p(out)
    d.w_bstride = 0 if w_pp.shape[0] == 1 else w_pp.shape[1]
    d.out_scale, d.bias, d.noise, d.noise_w = _f32(out_scale), _f32(bias), _f32(noise), _f32(noise_w)
    d.B, d.H, d.W, d.Cin, d.Cout = B, H, W, Cin, cout
    d.noise_batch = 1 if noise is None else noise.shape[0]
    d.noise_w_per_channel = 0 if (noise_w is None or noise_w.numel() == 1) else 1
    d.act, d.bias_scale, d.gain = act, bias_scale, gain
    if dgrad:
        dot_src = _mask_as_dot_src("conv_pp", relu_mask, dot_src, prep)
        d.dgrad, d.in_s2d, d.in_t2d, d.mask_relu = 1, 1 if in_s2d else 0, 1 if in_t2d else 0, 0 if relu_mask is None else 1
        d.dot_src, d.addend, d.add_scale = _p(dot_src), _p(addend), float(add_scale)
        st, nslot, _ = _stats_target(stats, B, H, W, 32, x.device, spread_plain=False)
        if stats is None:
            nslot = _stats_slots(B, H, W, 32)         # (the sums of a `prep` without stats are spread all the same)
        d.stats, d.stats_slots = _f32(st), nslot
        if prep is not None:
            if dot_src is None:
                raise DgeError("conv_pp: prep needs dot_src")
            _set_prep(d, prep, nslot)
    elif in_s2d or in_t2d or dot_src is not None or addend is not None or stats is not None or prep is not None or relu_mask is not None:
        raise DgeError("conv_pp: in_s2d / dot_src / addend / stats / prep / relu_mask need dgrad=True")
    macs = 9.0 * (Cin // 4 if (in_s2d or in_t2d) else Cin) * cout * H * W         # (an up layer's adjoint counts as the 3x3 transposed conv it replaces)
    _launch(lib().dge_conv_pp, (C.byref(d), _stream()), "dge_conv_pp", macs * B, (B, H, W, Cin, cout, 3, False, bool(in_s2d or in_t2d)),
            (x, out, w_pp, dot_src, addend), log=True)
    return out


def torgb(x, wrgb, style, bias, prev, wscale):
    B, H, W, Cin = x.shape
    img = torch.empty((B, 3, H, W), dtype=torch.float32, device=x.device)
    check(lib().dge_torgb(_p(x), _f32(wrgb), _f32(style), _f32(bias), _f32(prev), _p(img), B, H, W, Cin, float(wscale),
                          dtype_of(x), _stream()), "dge_torgb")
    return img


def nchw_to_nhwc(src, B, dtype):
    """src: [sB, C, H, W] f32 with sB in {1, B} -> [B, H, W, C] of dtype."""
    sB, Cc, H, W = src.shape
    dst = torch.empty((B, H, W, Cc), dtype=tdtype(dtype), device=src.device)
    check(lib().dge_nchw_to_nhwc(_f32(src.contiguous()), _p(dst), B, Cc, H * W, sB, dtype, _stream()), "dge_nchw_to_nhwc")
    return dst


def nhwc_to_nchw(src):
    B, H, W, Cc = src.shape
    dst = torch.empty((B, Cc, H, W), dtype=torch.float32, device=src.device)
    check(lib().dge_nhwc_to_nchw(_p(src), _p(dst), B, Cc, H * W, dtype_of(src), _stream()), "dge_nhwc_to_nchw")
    return dst


# ------------------------------------------------------------------ encoder streaming ops
def fromrgb(img, w, bias, dtype, stats=None, img4=False):
    """img4: also return the image in pixel-major form [B,H,W,4] f32 = (r, g, b, 1) (the backward's fused FromRGB reduction reads it)"""
    B, _, H, W = img.shape
    Cc = w.shape[0]
    y = torch.empty((B, H, W, Cc), dtype=tdtype(dtype), device=img.device)
    i4 = torch.empty((B, H, W, 4), dtype=torch.float32, device=img.device) if img4 else None
    check(lib().dge_fromrgb2(_f32(img.contiguous()), _f32(w.reshape(Cc, 3)), _f32(bias), _p(y), _f32(stats), _f32(i4), B, H * W, Cc,
                             dtype, _stream()), "dge_fromrgb")
    return (y, i4) if img4 else y


def stats_finalize(stats, npix, eps=1e-8, musig_out=None):
    """stats: [B,C,2] tensor or SlotStats; musig_out: optional preallocated [B, 2C] destination of (mean, std)"""
    nslot = 1
    if isinstance(stats, SlotStats):
        B, Cc, nslot, stats = stats.B, stats.C, stats.nslot, stats.buf
    else:
        B, Cc, _ = stats.shape
    musig = torch.empty((B, 2 * Cc), dtype=torch.float32, device=stats.device) if musig_out is None else musig_out
    sc = torch.empty((B, Cc), dtype=torch.float32, device=stats.device)
    sh = torch.empty((B, Cc), dtype=torch.float32, device=stats.device)
    check(lib().dge_stats_finalize_slots(_f32(stats), nslot, _p(musig), _p(sc), _p(sh), B, Cc, int(npix), float(eps), _stream()),
          "dge_stats_finalize")
    return musig, sc, sh


def blend(x, z=None, sc=None, sh=None, pool=False, alpha=1.0, beta=0.0, stats=None, mask=False):
    """mask=True (pooling blend without sc / sh): also returns the sign mask of x for act_bwd_mask -> (y, mask)"""
    B, H, W, Cc = x.shape
    OH, OW = (H // 2, W // 2) if pool else (H, W)
    y = torch.empty((B, OH, OW, Cc), dtype=x.dtype, device=x.device)
    if mask:
        if not pool or sc is not None or sh is not None:
            raise DgeError("blend: the sign mask is offered for the plain pooling blend")
        ep = 8 if x.dtype == torch.bfloat16 else 4
        m = torch.empty((B, OH * OW, Cc // ep), dtype=torch.int32, device=x.device)
        check(lib().dge_blend_pool_mask(_p(x), _p(z), _p(y), _f32(stats), _p(m), B, OH, OW, Cc, float(alpha), float(beta), dtype_of(x),
                                        _stream()), "dge_blend_pool_mask")
        return y, m
    check(lib().dge_blend(_p(x), _p(z), _p(y), _f32(sc), _f32(sh), _f32(stats), B, OH, OW, Cc, 1 if pool else 0,
                          float(alpha), float(beta), dtype_of(x), _stream()), "dge_blend")
    return y


# ------------------------------------------------------------------ StyleGAN2 backward ops
def modconv_bwd_prep(gx, x, d, noise, gain, R=None):
    B, H, W, Cc = x.shape
    gy = torch.empty_like(x)
    check(lib().dge_modconv_bwd_prep(_p(gx), _p(x), _f32(d), _f32(noise), _p(gy), _f32(R), B, H * W, Cc,
                                     1 if noise is None else noise.shape[0], float(gain), dtype_of(x), _stream()),
          "dge_modconv_bwd_prep")
    return gy


def torgb_bwd_prep(gimg, x, wrgb, style, wscale, noise, ns, gain):
    """top of the synthesis backward: toRGB adjoint + tail backward of the layer in one pass -> (g_z, gs [B,C], P [B,C,2])"""
    B, H, W, Cc = x.shape
    gz = torch.empty_like(x)
    gs = zeros((B, Cc), x.device)
    P = zeros((B, Cc, 2), x.device)
    check(lib().dge_torgb_bwd_prep(_f32(gimg), _p(x), _f32(wrgb), _f32(style), _f32(noise), _f32(ns if noise is not None else None),
                                   1 if noise is None else noise.shape[0], _p(gz), _p(gs), _p(P), B, H * W, Cc, float(wscale),
                                   float(gain), dtype_of(x), _stream()), "dge_torgb_bwd_prep")
    return gz, gs, P


def demod_bwd_prep(P, d, bias, bscale=1.0):
    """t [B,C] from the fused tail-backward sums P (a [B,C,2] tensor or a SlotStats filled by conv2d(prep=...))"""
    B, Cc = d.shape
    nslot = 1
    if isinstance(P, SlotStats):
        nslot, P = P.nslot, P.buf
    t = torch.empty_like(d)
    check(lib().dge_demod_bwd_prep(_f32(P), nslot, _f32(d), _f32(bias), _p(t), B, Cc, float(bscale), _stream()), "dge_demod_bwd_prep")
    return t


def demod_bwd(R, d, bias, noise_strength, bscale=1.0):
    B, Cc = d.shape
    t = torch.empty_like(d)
    check(lib().dge_demod_bwd(_f32(R), _f32(d), _f32(bias), _f32(noise_strength), _p(t), B, Cc, float(bscale), _stream()),
          "dge_demod_bwd")
    return t


def linear_t(x, w, y, mul=None, scale=1.0, accumulate=False, incx=1, incy=1, ldx=None, ldy=None, B=None, O=None):
    """y[b, k*incy] (+)= scale * mul[b,k] * sum_o x[b, o*incx] * w[o, k].  x / y are given as tensors whose
    data_ptr is element (0,0); row strides default to tensor strides."""
    O_, K = w.shape
    B = x.shape[0] if B is None else B
    O = O_ if O is None else O
    ldx = x.stride(0) if ldx is None else ldx
    ldy = y.stride(0) if ldy is None else ldy
    check(lib().dge_linear_t(C.c_void_p(x.data_ptr()), ldx, incx, _f32(w), _f32(mul), C.c_void_p(y.data_ptr()), ldy, incy,
                             B, O, K, float(scale), 1 if accumulate else 0, _stream()), "dge_linear_t")
    _log_dense("dge_linear_t")
    return y


def fir_t2d(g, scale=None):
    """g [B,2H,2W,C] -> Z [B,H+1,W+1,4C] = scale * FIR^T(g) stored t-grid-to-depth (dge_fir_t2d): the input of conv2d(in_t2d=True)"""
    B, FH, FW, Cc = g.shape
    H, W = FH // 2, FW // 2
    z = torch.empty((B, H + 1, W + 1, 4 * Cc), dtype=g.dtype, device=g.device)
    check(lib().dge_fir_t2d(_p(g), _f32(scale), _p(z), B, H, W, Cc, dtype_of(g), _stream()), "dge_fir_t2d")
    return z


def s2_style_grads(blocks, g_wp, wscale):
    """blocks: list of dicts - conv block: P (SlotStats or [B,out_c,2]), st (SlotStats), d, s, bias, wsq, bscale, wstyle, row;
    toRGB block: gs, wstyle, row.  One launch for every style gradient of the synthesis backward (dge_s2_style_grads)."""
    from ._lib import S2GradEntry
    arr = (S2GradEntry * len(blocks))()
    B, nrows, K = g_wp.shape
    for e, blk in zip(arr, blocks):
        e.wstyle, e.row = _f32(blk["wstyle"]), int(blk["row"])
        if "gs" in blk:
            e.gs, e.in_c = _f32(blk["gs"]), blk["gs"].shape[1]
            continue
        P, st = blk["P"], blk["st"]
        e.nslot_p, e.nslot_s = 1, 1
        if isinstance(P, SlotStats):
            e.nslot_p, P = P.nslot, P.buf
        if isinstance(st, SlotStats):
            e.nslot_s, st = st.nslot, st.buf
        e.P, e.st, e.d, e.s, e.bias, e.wsq = _f32(P), _f32(st), _f32(blk["d"]), _f32(blk["s"]), _f32(blk["bias"]), _f32(blk["wsq"])
        e.out_c, e.in_c = blk["d"].shape[1], blk["s"].shape[1]
        e.bscale = float(blk["bscale"])
    check(lib().dge_s2_style_grads(arr, len(blocks), _p(g_wp), B, nrows, K, float(wscale), _stream()), "dge_s2_style_grads")
    return g_wp


def s2_style_grads_s(blocks, B):
    """The S-space ending of the synthesis backward (dge_s2_style_grads_s): every block of the list stores its style gradient to
    `out`, its own contiguous [B,in_c] slice of the style-gradient buffer.  Blocks are dicts - conv block: P, st, d, s, bias, wsq,
    bscale (as s2_style_grads takes them); finished block: st alone (SlotStats or [B,in_c,2]); toRGB block: gs.  One launch."""
    from ._lib import S2SGradEntry
    arr = (S2SGradEntry * len(blocks))()
    for e, blk in zip(arr, blocks):
        out = blk["out"]
        if out.dtype != torch.float32 or not out.is_contiguous() or out.shape[0] != B:
            raise DgeError("s2_style_grads_s: `out` is a contiguous float32 [B,in_c] slice")
        e.out, e.in_c = _p(out), out.shape[1]
        if "gs" in blk:
            if tuple(blk["gs"].shape) != tuple(out.shape):
                raise DgeError("s2_style_grads_s: gs and out have one shape")
            e.gs = _f32(blk["gs"])
            continue
        st = blk["st"]
        e.nslot_p, e.nslot_s = 1, 1
        if isinstance(st, SlotStats):
            e.nslot_s, st = st.nslot, st.buf
        if st.numel() != e.nslot_s * B * e.in_c * 2:
            raise DgeError("s2_style_grads_s: st holds [nslot][B,in_c,2]")
        e.st = _f32(st)
        if "P" not in blk:
            continue
        P = blk["P"]
        if isinstance(P, SlotStats):
            e.nslot_p, P = P.nslot, P.buf
        e.out_c = blk["d"].shape[1]
        if blk["s"].shape[1] != e.in_c or P.numel() != e.nslot_p * B * e.out_c * 2 or blk["wsq"].numel() != e.out_c * e.in_c:
            raise DgeError("s2_style_grads_s: a conv block's P [nslot][B,out_c,2], d [B,out_c], s [B,in_c], wsq [out_c,in_c] disagree")
        e.P, e.d, e.s, e.bias, e.wsq = _f32(P), _f32(blk["d"]), _f32(blk["s"]), _f32(blk["bias"]), _f32(blk["wsq"])
        e.bscale = float(blk["bscale"])
    check(lib().dge_s2_style_grads_s(arr, len(blocks), int(B), _stream()), "dge_s2_style_grads_s")
    log_kernel()


def torgb_bwd(gimg, x, wrgb, style, wscale):
    B, H, W, Cc = x.shape
    gx = torch.empty_like(x)
    gs = zeros((B, Cc), x.device)
    check(lib().dge_torgb_bwd(_f32(gimg), _p(x), _f32(wrgb), _f32(style), _p(gx), _p(gs), B, H * W, Cc, float(wscale),
                              dtype_of(x), _stream()), "dge_torgb_bwd")
    return gx, gs


def up2_bwd(g):
    B, Cc, H, W = g.shape
    out = torch.empty((B, Cc, H // 2, W // 2), dtype=torch.float32, device=g.device)
    check(lib().dge_up2_bwd(_f32(g), _p(out), B * Cc, H // 2, W // 2, _stream()), "dge_up2_bwd")
    return out


# ------------------------------------------------------------------ encoder backward ops
def conv_wgrad(g, x, dw, in_scale=None, in_shift=None):
    """dw [Cout,Cin,k,k] f32 (pre-zeroed or accumulating) += wgrad(g, x*in_scale+in_shift)."""
    B, H, W, Cin = x.shape
    cout, _, k, _ = dw.shape
    check(lib().dge_conv_wgrad(_p(g), _p(x), _f32(in_scale), _f32(in_shift), _f32(dw), B, H, W, cout, Cin, k, dtype_of(x),
                               _stream()), "dge_conv_wgrad")
    return dw


def conv_wgrad_dots(g, x, dw, in_scale, in_shift, w, dots):
    """conv_wgrad that also fills `dots` (SlotStats(B, Cin)) with (sum g_x*x, sum g_x) of the layer's data gradient g_x, where the
    streaming weight-gradient kernel covers the shape: returns True then; False (nothing launched) otherwise."""
    B, H, W, Cin = x.shape
    cout = dw.shape[0]
    if dw.shape[2] != 3 or is_deterministic():
        return False
    nslot = max(1, min(16, (H * W) // 4096))
    buf = dots.alloc(nslot)
    r = lib().dge_conv_wgrad_dots(_p(g), _p(x), _f32(in_scale), _f32(in_shift), _f32(dw), _f32(w.detach()), _f32(buf), nslot, B, H, W, cout, Cin,
                                  dtype_of(x), _stream())
    if r == 1:
        dots.buf, dots.nslot = None, 1
        return False
    check(r, "dge_conv_wgrad_dots")
    return True


class DeferredSums:
    """Planar slot sums whose results nobody reads before the end of a backward: collected, then run as ONE launch
    (dge_sum_slots_planar_multi) by flush()."""

    def __init__(self):
        self.items = []

    def add(self, part, red):
        self.items.append((part, red))
        if len(self.items) == 32:
            self.flush()
        return red

    def flush(self):
        if not self.items:
            return
        from ._lib import SumPlanarEntry
        arr = (SumPlanarEntry * len(self.items))()
        for e, (part, red) in zip(arr, self.items):
            e.partial, e.out = _p(part), _p(red)
            e.nslot, e.C, e.NS = part.shape
        check(lib().dge_sum_slots_planar_multi(arr, len(self.items), _stream()), "dge_sum_slots_planar_multi")
        self.items = []


def _sum_planar(part, red, defer=None):
    """part [B, C, NS] per-sample sums -> red [NS, C] (each reduction a contiguous vector)."""
    if defer is not None:
        return defer.add(part, red)
    B, Cc, NS = part.shape
    check(lib().dge_sum_slots_planar(_p(part), _p(red), B, Cc, NS, _stream()), "dge_sum_slots_planar")
    return red


def act_bwd(gup, a, noise=None, pool=False, scale=1.0, red=None, slope=0.2, planar=False, defer=None):
    """red [C, 2|3] (pre-zeroed; [2|3, C] when planar) receives the batch-summed reductions: the kernel writes per-sample
    partial sums (no cross-sample contention on the atomics) that are added over the batch here."""
    B, H, W, Cc = a.shape
    gpre = torch.empty_like(a)
    ncol = 2 if red is None else (red.shape[0] if planar else red.shape[-1])
    part = zeros((B, Cc, ncol), a.device) if red is not None else None
    check(lib().dge_act_bwd(_p(gup), _p(a), _f32(noise), _p(gpre), _f32(part), ncol, B, H, W, Cc,
                            1 if pool else 0, float(scale), float(slope), dtype_of(a), _stream()), "dge_act_bwd")
    if red is not None:
        _sum_planar(part, red, defer) if planar else _sum_over_batch(part, red)
    return gpre


def act_bwd_mask(gup, mask, noise, scale=1.0, red=None, slope=0.2, planar=False, defer=None):
    """act_bwd(pool=True) from the sign mask of blend(..., mask=True): gup [B,H/2,W/2,C] -> g_pre [B,H,W,C]"""
    B, UH, UW, Cc = gup.shape
    H, W = 2 * UH, 2 * UW
    gpre = torch.empty((B, H, W, Cc), dtype=gup.dtype, device=gup.device)
    ncol = 2 if red is None else (red.shape[0] if planar else red.shape[-1])
    part = zeros((B, Cc, ncol), gup.device) if red is not None else None
    check(lib().dge_act_bwd_mask(_p(gup), _p(mask), _f32(noise), _p(gpre), _f32(part), ncol, B, H, W, Cc, float(scale), float(slope),
                                 dtype_of(gup), _stream()), "dge_act_bwd_mask")
    if red is not None:
        _sum_planar(part, red, defer) if planar else _sum_over_batch(part, red)
    return gpre


def in_bwd_coef(dots, gms, musig, sc, sh, npix):
    B, Cc = sc.shape
    coef = torch.empty((B, Cc, 3), dtype=torch.float32, device=sc.device)
    nslot = 1
    if isinstance(dots, SlotStats):
        nslot, dots = dots.nslot, dots.buf
    check(lib().dge_in_bwd_coef_slots(_f32(dots), nslot, _f32(gms), _f32(musig), _f32(sc), _f32(sh), _p(coef), B, Cc, int(npix),
                                      _stream()), "dge_in_bwd_coef")
    return coef


def in_bwd(gy, x, coef, extra=None, extra_pool=False, extra_scale=1.0, noise=None, act=False, red=None, planar=False, defer=None):
    """red [C, 2] (or [2, C] when planar).  `coef`: [B,C,3] from in_bwd_coef, or the tuple (dots, gms, musig, sc, sh, npix) of its
    arguments - the launch then computes the coefficients itself (dge_in_bwd_fused, C <= 512)."""
    B, H, W, Cc = x.shape
    gout = torch.empty_like(x)
    part = zeros((B, Cc, 2), x.device) if red is not None else None
    if isinstance(coef, tuple) and Cc > 512:
        coef = in_bwd_coef(*coef)
    if isinstance(coef, tuple):
        dots, gms, musig, sc, sh, npix = coef
        nslot = 1
        if isinstance(dots, SlotStats):
            nslot, dots = dots.nslot, dots.buf
        check(lib().dge_in_bwd_fused(_p(gy), _p(x), _f32(dots), nslot, _f32(gms), _f32(musig), _f32(sc), _f32(sh), int(npix), _p(extra),
                                     _f32(noise), _p(gout), _f32(part), B, H, W, Cc, 1 if extra_pool else 0, float(extra_scale),
                                     1 if act else 0, dtype_of(x), _stream()), "dge_in_bwd_fused")
    else:
        check(lib().dge_in_bwd(_p(gy), _p(x), _f32(coef), _p(extra), _f32(noise), _p(gout), _f32(part), B, H, W, Cc,
                               1 if extra_pool else 0, float(extra_scale), 1 if act else 0, dtype_of(x), _stream()), "dge_in_bwd")
    if red is not None:
        _sum_planar(part, red, defer) if planar else _sum_over_batch(part, red)
    return gout


def in_bwd_fromrgb(gy, x0, coef, img, extra=None, extra_pool=False, extra_scale=1.0, defer=None):
    """Last step of the encoder backward: in_bwd (coefficients computed in the launch, `coef` = (dots, gms, musig, sc, sh, npix))
    on the FromRGB output x0 with the FromRGB parameter gradients reduced from the result in registers -> [4, C] (planar: weight
    gradient rows 0..2, bias gradient row 3).  The gradient w.r.t. x0 is never stored."""
    B, H, W, Cc = x0.shape
    dots, gms, musig, sc, sh, npix = coef
    nslot = 1
    if isinstance(dots, SlotStats):
        nslot, dots = dots.nslot, dots.buf
    part = zeros((B, Cc, 4), x0.device)
    check(lib().dge_in_bwd_fromrgb(_p(gy), _p(x0), _f32(dots), nslot, _f32(gms), _f32(musig), _f32(sc), _f32(sh), int(npix), _p(extra),
                                   _f32(img.contiguous()), _p(part), B, H, W, Cc, 1 if extra_pool else 0, float(extra_scale),
                                   dtype_of(x0), _stream()), "dge_in_bwd_fromrgb")
    return _sum_planar(part, torch.empty((4, Cc), dtype=torch.float32, device=x0.device), defer)


def in_bwd_fromrgb_img_supported(Cc, dtype):
    """Whether dge_in_bwd_fromrgb_img takes the channel count (its own checks: C <= 512, 16-byte chunks that tile a workgroup)."""
    cpt, rem = divmod(int(Cc), 8 if dtype == BF16 else 4)
    return rem == 0 and 1 <= cpt <= 256 and 256 % cpt == 0 and Cc <= 512


def in_bwd_fromrgb_img(gy, x0, coef, w, img=None, extra=None, extra_pool=False, extra_scale=1.0, defer=None):
    """Last step of the encoder backward when the image carries a gradient: in_bwd (`coef` = (dots, gms, musig, sc, sh, npix)) on the
    FromRGB output x0, the FromRGB data gradient of the result -> g_img [B,3,H,W] f32 and, with `img`, the FromRGB parameter
    gradients [4, C] as in_bwd_fromrgb gives them (None without).  The gradient w.r.t. x0 is never stored.  w: FromRGB's weight."""
    B, H, W, Cc = x0.shape
    dots, gms, musig, sc, sh, npix = coef
    nslot = 1
    if isinstance(dots, SlotStats):
        nslot, dots = dots.nslot, dots.buf
    gimg = torch.empty((B, 3, H, W), dtype=torch.float32, device=x0.device)
    part = zeros((B, Cc, 4), x0.device) if img is not None else None
    check(lib().dge_in_bwd_fromrgb_img(_p(gy), _p(x0), _f32(dots), nslot, _f32(gms), _f32(musig), _f32(sc), _f32(sh), int(npix), _p(extra),
                                       _f32(w.reshape(Cc, 3).contiguous()), _f32(img.contiguous()) if img is not None else None, _p(part),
                                       _p(gimg), B, H, W, Cc, 1 if extra_pool else 0, float(extra_scale), dtype_of(x0), _stream()),
          "dge_in_bwd_fromrgb_img")
    log_kernel()
    if part is None:
        return gimg, None
    return gimg, _sum_planar(part, torch.empty((4, Cc), dtype=torch.float32, device=x0.device), defer)


def affine_bwd_fromrgb_img_supported(Cc, dtype):
    """Whether dge_affine_bwd_fromrgb_img takes the channel count: the rule of in_bwd_fromrgb_img_supported (the same kernel)."""
    return in_bwd_fromrgb_img_supported(Cc, dtype)


def affine_bwd_fromrgb_img(gy, x0, a, w, img=None, extra=None, extra_pool=False, extra_scale=1.0, defer=None):
    """Last step of the E_BIG backward when the image carries a gradient: g = a * gy (+ extra_scale * extra) on the FromRGB output
    x0 (a [B,C]: the conditional batch norm's scale), the FromRGB data gradient of the result -> g_img [B,3,H,W] f32 and, with `img`,
    the FromRGB parameter gradients [4, C] (planar; None without).  The gradient w.r.t. x0 is never stored.  w: FromRGB's weight."""
    B, H, W, Cc = x0.shape
    if tuple(a.shape) != (B, Cc):
        raise DgeError(f"affine_bwd_fromrgb_img: a {tuple(a.shape)} is not [B={B}, C={Cc}]")
    gimg = torch.empty((B, 3, H, W), dtype=torch.float32, device=x0.device)
    part = zeros((B, Cc, 4), x0.device) if img is not None else None
    check(lib().dge_affine_bwd_fromrgb_img(_p(gy), _p(x0), _f32(a.float().contiguous()), _p(extra), _f32(w.reshape(Cc, 3).contiguous()),
                                           _f32(img.contiguous()) if img is not None else None, _p(part), _p(gimg), B, H, W, Cc,
                                           1 if extra_pool else 0, float(extra_scale), dtype_of(x0), _stream()),
          "dge_affine_bwd_fromrgb_img")
    log_kernel()
    if part is None:
        return gimg, None
    return gimg, _sum_planar(part, torch.empty((4, Cc), dtype=torch.float32, device=x0.device), defer)


def conv_pool_supported(B, H, W, cin, cout, ksize, dtype):
    return bool(lib().dge_conv_pool_supported(B, H, W, cin, cout, ksize, dtype))


def conv_rgb_supported(B, H, W, cin, cout, ksize, dtype):
    return bool(lib().dge_conv_rgb_supported(B, H, W, cin, cout, ksize, dtype))


def rgb_upsample_add(img, prev):
    """img [B,3,H,W] += up2(prev [B,3,H/2,W/2]) in place (the skip connection of SynthesisModule.forward :517-522)"""
    B, Cc, H, W = img.shape
    check(lib().dge_rgb_upsample_add(_p(img), _f32(prev), B * Cc, H, W, _stream()), "dge_rgb_upsample_add")
    return img


def chan_sum(x, scale=1.0):
    B, H, W, Cc = x.shape
    part = zeros((B, Cc), x.device)
    check(lib().dge_chan_sum(_p(x), _p(part), B, H * W, Cc, float(scale), dtype_of(x), _stream()), "dge_chan_sum")
    return _sum_over_batch(part)


def fromrgb_bwd(gx, x0, img, planar=False, defer=None):
    """-> [C, 4] (weight gradient columns 0..2, bias gradient column 3); planar: [4, C]"""
    B, H, W, Cc = x0.shape
    part = zeros((B, Cc, 4), x0.device)
    check(lib().dge_fromrgb_bwd(_p(gx), _p(x0), _f32(img.contiguous()), _p(part), B, H * W, Cc, dtype_of(x0), _stream()),
          "dge_fromrgb_bwd")
    if planar:
        return _sum_planar(part, torch.empty((4, Cc), dtype=torch.float32, device=x0.device), defer)
    return _sum_over_batch(part)


def dense_wgrad(gy, x, gw, gb=None, accumulate=False):
    """gy: [B,O] view (row stride free), x: [B,I]; gw [O,I], gb [O]."""
    B, O = gy.shape
    I = x.shape[1]
    check(lib().dge_dense_wgrad(C.c_void_p(gy.data_ptr()), gy.stride(0), C.c_void_p(x.data_ptr()), x.stride(0), _f32(gw),
                                _f32(gb), B, O, I, 1 if accumulate else 0, _stream()), "dge_dense_wgrad")
    _log_dense("dge_dense_wgrad")
    return gw, gb


def _rows_view(t, what):
    """(pointer, batch stride, row stride, rows) of a W+ tensor [B, rows, O] f32 with unit inner stride (views allowed)"""
    if not t.is_cuda or t.dtype != torch.float32 or t.ndim != 3 or t.stride(2) != 1:
        raise DgeError(f"{what}: expected a float32 GPU tensor [B, rows, O] with unit inner stride")
    return C.c_void_p(t.data_ptr()), t.stride(0), t.stride(1), t.shape[1]


def heads_fwd(tab, n, musig_all, w):
    """Every head of a one-column table (enc_steps.heads_table) in one launch: w[b, col] = musig_l @ W_l^T + b_l into w [B, 2L, O]."""
    check(lib().dge_heads_fwd(_p(tab), n, _f32(musig_all), _p(w), w.stride(0), w.shape[0], w.shape[2], _stream()), "dge_heads_fwd")
    return w


def heads_bwd(tab, n, max_I, g, musig_all, gms_all, gw_all, gb_all):
    """Backward of heads_fwd from g = dL/dw [B, 2L, O] (rows O apart, batch stride free): gms_all, gw_all and gb_all, flat by the
    table's moff / woff / boff.  Two launches, no atomics."""
    check(lib().dge_heads_bwd(_p(tab), n, int(max_I), _f32(g), g.stride(0), _f32(musig_all), _p(gms_all), _p(gw_all), _p(gb_all),
                              g.shape[0], g.shape[2], _stream()), "dge_heads_bwd")
    return gms_all


def heads_rows_fwd(tab, n, musig_all, w):
    """Every head of a row-list table (enc_steps.heads_table) in one launch: w[b, row_a | row_b] = musig_l @ W_l^T + b_l,
    written in place into w [B, rows, O] (a view with unit inner stride works); the bits of linear() per head."""
    wp, ldb, ldr, rows = _rows_view(w, "heads_rows_fwd")
    check(lib().dge_heads_rows_fwd(_p(tab), n, _f32(musig_all), wp, ldb, ldr, rows, w.shape[0], w.shape[2], _stream()), "dge_heads_rows_fwd")
    _log_dense("dge_heads_rows_fwd")
    return w


def heads_rows_bwd(tab, n, max_I, g, musig_all, gms_all, gw_all=None, gb_all=None):
    """Backward of heads_rows_fwd from g = dL/dw [B, rows, O] (row strides free): gms_all (flat, by the table's moff) always; gw_all /
    gb_all (flat, by woff / boff) when given - without them the data gradient alone, one launch.  No atomics."""
    gp, ldb, ldr, rows = _rows_view(g, "heads_rows_bwd")
    check(lib().dge_heads_rows_bwd(_p(tab), n, int(max_I), gp, ldb, ldr, rows, _f32(musig_all), _f32(gms_all), _f32(gw_all), _f32(gb_all),
                                   g.shape[0], g.shape[2], _stream()), "dge_heads_rows_bwd")
    _log_dense("dge_heads_rows_bwd")
    return gms_all


def scale_(t, factor):
    """in-place t *= factor on the device (dge_axpy_scalar)."""
    check(lib().dge_axpy_scalar(_f32(t), None, _p(t), t.numel(), float(factor), 0, _stream()), "dge_axpy_scalar")
    return t


# ------------------------------------------------------------------ StyleGAN1 ops
def blur_noise_act(x, noise, noise_w, bias, blur=True, stats=None, act=True):
    B, H, W, Cc = x.shape
    y = torch.empty_like(x)
    check(lib().dge_blur_noise_act(_p(x), _f32(noise), _f32(noise_w), _f32(bias), _p(y), _f32(stats), B, H, W, Cc,
                                   1 if blur else 0, 1 if noise is None else noise.shape[0], 1 if act else 0, dtype_of(x),
                                   _stream()), "dge_blur_noise_act")
    return y


def affine_compose(sc, sh, style):
    B, Cc = sc.shape
    a = torch.empty_like(sc)
    b = torch.empty_like(sc)
    check(lib().dge_affine_compose(_f32(sc), _f32(sh), _f32(style), _p(a), _p(b), B, Cc, _stream()), "dge_affine_compose")
    return a, b


def lerp_layers(w, avg, coefs):
    """w [B,D]; avg [D] or [L,D]; coefs [L] -> [B,L,D]"""
    B, D = w.shape
    L = coefs.numel()
    out = torch.empty((B, L, D), dtype=torch.float32, device=w.device)
    stride = D if avg.numel() == L * D else 0
    check(lib().dge_lerp_layers(_f32(w), _f32(avg.contiguous()), stride, _f32(coefs.contiguous()), _p(out), B, L, D, _stream()),
          "dge_lerp_layers")
    return out


# ------------------------------------------------------------------ PGGAN ops
def pixelnorm_nhwc(x, eps=1e-8):
    B, H, W, Cc = x.shape
    y = torch.empty_like(x)
    check(lib().dge_pixelnorm_nhwc(_p(x), _p(y), B * H * W, Cc, float(eps), dtype_of(x), _stream()), "dge_pixelnorm_nhwc")
    return y


# ------------------------------------------------------------------ BigGAN ops
def cbn_affine(scale, offset, mean, var, eps):
    """scale/offset: [B,C] (or [1,C] batch-shared); mean/var: [C] -> a, b [B,C]"""
    B, Cc = scale.shape
    a = torch.empty((B, Cc), dtype=torch.float32, device=scale.device)
    b = torch.empty_like(a)
    # scale / offset may be column slices of one wide [B, sum C] matrix (all conditional-BN linears of a module in one launch)
    ld = scale.stride(0) if B > 1 else Cc
    if scale.dtype != torch.float32 or offset.dtype != torch.float32 or scale.stride(1) != 1 or offset.stride(1) != 1 or \
            (B > 1 and offset.stride(0) != ld):
        raise DgeError("cbn_affine: scale / offset must be float32 rows with unit inner stride and a common row stride")
    check(lib().dge_cbn_affine(C.c_void_p(scale.data_ptr()), C.c_void_p(offset.data_ptr()), ld, _f32(mean.contiguous()),
                               _f32(var.contiguous()), float(eps), _p(a), _p(b), B, Cc, _stream()), "dge_cbn_affine")
    return a, b


def slice_up(x, cout, up):
    B, H, W, Cin = x.shape
    f = 2 if up else 1
    y = torch.empty((B, H * f, W * f, cout), dtype=x.dtype, device=x.device)
    check(lib().dge_slice_up(_p(x), _p(y), B, H, W, Cin, cout, 1 if up else 0, dtype_of(x), _stream()), "dge_slice_up")
    return y


def attention(q, k, v):
    """q [B,N,D], k [B,M,D], v [B,M,DV] -> [B,N,DV] (softmax over the M keys, no scaling)"""
    B, N, D = q.shape
    M, DV = k.shape[1], v.shape[2]
    o = torch.empty((B, N, DV), dtype=q.dtype, device=q.device)
    check(lib().dge_attention(_p(q), _p(k), _p(v), _p(o), B, N, M, D, DV, dtype_of(q), _stream()), "dge_attention")
    return o


def maxpool2(x):
    B, H, W, Cc = x.shape
    y = torch.empty((B, H // 2, W // 2, Cc), dtype=x.dtype, device=x.device)
    check(lib().dge_maxpool2(_p(x), _p(y), B, H, W, Cc, dtype_of(x), _stream()), "dge_maxpool2")
    return y


def rgb_tanh(x):
    B, H, W, Cc = x.shape
    img = torch.empty((B, 3, H, W), dtype=torch.float32, device=x.device)
    check(lib().dge_rgb_tanh(_p(x), _p(img), B, H * W, Cc, dtype_of(x), _stream()), "dge_rgb_tanh")
    return img


def sg1_in_bwd_coef(dots, sc, sh, style, npix):
    """-> (coef [B,C,3], gstyle [B,2C]) of the instance-norm + style_mod backward (dge_sg1_in_bwd_coef)."""
    B, Cc = sc.shape
    coef = torch.empty((B, Cc, 3), dtype=torch.float32, device=sc.device)
    gstyle = torch.empty((B, 2 * Cc), dtype=torch.float32, device=sc.device)
    check(lib().dge_sg1_in_bwd_coef(_f32(dots), _f32(sc), _f32(sh), _f32(style), _p(coef), _p(gstyle), B, Cc, int(npix), _stream()),
          "dge_sg1_in_bwd_coef")
    return coef, gstyle


def dot_stats(g, x):
    B, H, W, Cc = x.shape
    st = zeros((B, Cc, 2), x.device)
    check(lib().dge_dot_stats(_p(g), _p(x), _p(st), B, H * W, Cc, dtype_of(x), _stream()), "dge_dot_stats")
    return st


def nearest_up2_bwd(ghi, x=None):
    """Adjoint of the nearest x2 upsample; with x also the dot statistics (sum g*x, sum g) [B,C,2]."""
    B, H2, W2, Cc = ghi.shape
    glow = torch.empty((B, H2 // 2, W2 // 2, Cc), dtype=ghi.dtype, device=ghi.device)
    st = zeros((B, Cc, 2), ghi.device) if x is not None else None
    check(lib().dge_nearest_up2_bwd(_p(ghi), _p(x), _p(glow), _f32(st), B, H2 // 2, W2 // 2, Cc, dtype_of(ghi), _stream()),
          "dge_nearest_up2_bwd")
    return glow, st


def fromrgb_dgrad(gx, x0, w):
    """Gradient of FromRGB w.r.t. its input image -> [B,3,H,W] f32."""
    B, H, W, Cc = x0.shape
    gimg = torch.empty((B, 3, H, W), dtype=torch.float32, device=x0.device)
    check(lib().dge_fromrgb_dgrad(_p(gx), _p(x0), _f32(w.reshape(Cc, 3).contiguous()), _p(gimg), B, H * W, Cc, dtype_of(x0), _stream()),
          "dge_fromrgb_dgrad")
    return gimg


def nearest_up2(x, scale=1.0):
    B, H, W, Cc = x.shape
    y = torch.empty((B, 2 * H, 2 * W, Cc), dtype=x.dtype, device=x.device)
    check(lib().dge_nearest_up2(_p(x), _p(y), B, H, W, Cc, float(scale), dtype_of(x), _stream()), "dge_nearest_up2")
    return y


def linear_rows(x, ldx_b, row_xoff, w, bias, y, row_ybase, row_ybstride, B, wscale, bscale, add):
    R, K = w.shape
    check(lib().dge_linear_rows(_f32(x), int(ldx_b), _p(row_xoff), _f32(w), _f32(bias), _p(y), _p(row_ybase), _p(row_ybstride), B, R, K,
                                float(wscale), float(bscale), float(add), _stream()), "dge_linear_rows")
    return y


def demod_rows(s_all, wsq_cat, row_woff, row_sbase, row_cin, d_all, row_dbase, row_dbstride, B, eps):
    R = row_woff.numel()
    check(lib().dge_demod_rows(_f32(s_all), _f32(wsq_cat), _p(row_woff), _p(row_sbase), _p(row_cin), _p(d_all), _p(row_dbase),
                               _p(row_dbstride), B, R, float(eps), _stream()), "dge_demod_rows")
    return d_all


def pixelnorm_nhwc_bwd(gy, x, eps=1e-8):
    """x: [..., C] channel-last (NHWC activations, or [B,1,1,D] latent rows in f32)."""
    Cc = x.shape[-1]
    gx = torch.empty_like(x)
    check(lib().dge_pixelnorm_nhwc_bwd(_p(gy), _p(x), _p(gx), x.numel() // Cc, Cc, float(eps), dtype_of(x), _stream()), "dge_pixelnorm_nhwc_bwd")
    return gx


def pixelnorm_act_bwd_supported(Cc, dtype):
    """Whether dge_pixelnorm_act_bwd takes the channel count: dge_pixelnorm_nhwc_bwd's rule (a power-of-two number of 16-byte
    chunks, at most two per lane of a wave)."""
    chunks, rem = divmod(int(Cc), 8 if dtype == BF16 else 4)
    return rem == 0 and chunks >= 1 and chunks & (chunks - 1) == 0 and chunks <= 128


def pixelnorm_act_bwd(g, x, up=False, act=True, eps=1e-8):
    """pixelnorm_nhwc_bwd(g, x) times lrelu'(x) (`act`) in one launch; `up`: g is [B,2H,2W,C] and is first summed over its 2x2
    blocks in f32 (nearest_up2_bwd).  x [B,H,W,C]: the activation the pixel norm read, itself the output of a leaky-relu(0.2)."""
    B, H, W, Cc = x.shape
    if tuple(g.shape) != ((B, 2 * H, 2 * W, Cc) if up else (B, H, W, Cc)) or g.dtype != x.dtype:
        raise DgeError(f"pixelnorm_act_bwd: g {tuple(g.shape)} {g.dtype} does not go with x {tuple(x.shape)} {x.dtype} (up={bool(up)})")
    out = torch.empty_like(x)
    check(lib().dge_pixelnorm_act_bwd(_p(g), _p(x), _p(out), B, H, W, Cc, 1 if up else 0, 1 if act else 0, float(eps), dtype_of(x),
                                      _stream()), "dge_pixelnorm_act_bwd")
    log_kernel()
    return out


# ------------------------------------------------------------------ BigGAN-deep backward ops
def affine_relu_bwd(gu, x, a, b):
    """Backward of u = relu(a*x + b): -> (gx, stats [B,C,2] = (d/da, d/db))."""
    B, H, W, Cc = x.shape
    gx = torch.empty_like(x)
    st = zeros((B, Cc, 2), x.device)
    check(lib().dge_affine_relu_bwd(_p(gu), _p(x), _f32(a), _f32(b), _p(gx), _p(st), B, H * W, Cc, dtype_of(x), _stream()),
          "dge_affine_relu_bwd")
    return gx, st


def slice_up_bwd(gy, gx, up):
    """gx [B,H,W,Cin] += adjoint of slice_up applied to gy [B,H<<up,W<<up,Cout]."""
    B, H, W, Cin = gx.shape
    check(lib().dge_slice_up_bwd(_p(gy), _p(gx), B, H, W, Cin, gy.shape[3], 1 if up else 0, dtype_of(gx), _stream()), "dge_slice_up_bwd")
    return gx


def softmax_rows_(s):
    """in-place softmax over the last axis of a contiguous tensor"""
    M = s.shape[-1]
    check(lib().dge_softmax_rows(_p(s), s.numel() // M, M, dtype_of(s), _stream()), "dge_softmax_rows")
    return s


def softmax_rows_bwd_(p, gp):
    M = p.shape[-1]
    check(lib().dge_softmax_rows_bwd(_p(p), _p(gp), p.numel() // M, M, dtype_of(p), _stream()), "dge_softmax_rows_bwd")
    return gp


def rgb_tanh_bwd(gimg, img, Cc, dtype):
    B, _, H, W = img.shape
    gy = torch.empty((B, H, W, Cc), dtype=tdtype(dtype), device=img.device)
    check(lib().dge_rgb_tanh_bwd(_f32(gimg.contiguous()), _f32(img), _p(gy), B, H * W, Cc, dtype, _stream()), "dge_rgb_tanh_bwd")
    return gy


def maxpool2_bwd(gy, x, addend=None, relu=False):
    """gy [B,H/2,W/2,C], x [B,H,W,C] (the pooled tensor) -> gx [B,H,W,C] (+ addend); relu: times [x > 0] (the ReLU that made x)"""
    B, H, W, Cc = x.shape
    gx = torch.empty_like(x)
    fn = lib().dge_maxpool2_bwd_relu if relu else lib().dge_maxpool2_bwd
    check(fn(_p(gy), _p(x), _p(addend), _p(gx), B, H, W, Cc, dtype_of(x), _stream()), "dge_maxpool2_bwd")
    return gx


# ------------------------------------------------------------------ StyleGAN2 up layer at algorithmic cost
def upconv_supported(cin, cout, dtype):
    return bool(lib().dge_upconv_supported(int(cin), int(cout), int(dtype)))


def pack_upconv_weight(w, dtype=BF16, scale=1.0):
    """w: [Cout,Cin,3,3] f32 -> [9 (phase,tap) units, Cout, Cin] of `dtype` (dge_pack_upconv_weight)."""
    cout, cin = w.shape[0], w.shape[1]
    out = torch.empty((9, cout, cin), dtype=tdtype(dtype), device=w.device)
    check(lib().dge_pack_upconv_weight(_f32(w.detach().contiguous()), _p(out), cout, cin, float(scale), dtype, _stream()),
          "dge_pack_upconv_weight")
    return out


def upconv_fir(x, w_packed, cout, in_scale=None, out_scale=None, bias=None, bias_scale=1.0, noise=None, noise_w=None,
               act=ACT_NONE, gain=1.0):
    """x [B,H,W,Cin] -> y [B,2H,2W,cout]: conv_transpose2d(stride 2) + 4x4 FIR + noise / bias / activation in one kernel."""
    B, H, W, Cin = x.shape
    y = torch.empty((B, 2 * H, 2 * W, cout), dtype=x.dtype, device=x.device)
    nbs = 0 if (noise is None or noise.shape[0] == 1) else 4 * H * W
    nws = 0 if (noise_w is None or noise_w.numel() == 1) else 1
    _launch(lib().dge_upconv_fir, (_p(x), _p(w_packed), _p(y), _f32(in_scale), _f32(out_scale), _f32(noise), nbs, _f32(noise_w), nws,
                                   _f32(bias), float(bias_scale), float(gain), int(act), B, H, W, Cin, cout, dtype_of(x), _stream()),
            "dge_upconv_fir", 9.0 * Cin * cout * H * W * B, (B, H, W, Cin, cout, 3, "upfir", False), (x, y, w_packed))
    return y


# ------------------------------------------------------------------ data gradient of the narrow up layer as one stream
def up_dgrad_stream_supported(B, Hin, Win, cin, cout, dtype):
    """True when the data gradient of an up layer cin -> cout on the Hin x Win input grid runs on csrc/upconv_stream_bwd.hip:
    bf16, 64 -> 32, not in deterministic mode (its sums leave by atomics)."""
    return (not is_deterministic()) and bool(lib().dge_up_dgrad_stream_supported(int(B), int(Hin), int(Win), int(cin), int(cout), int(dtype)))


def pack_up_dgrad_stream(w, dtype=BF16, scale=1.0):
    """w: [Cout,Cin,3,3] f32 (the forward layer's parameter) -> [9 (ky,kx), Cin, Cout] bf16, element [3ky+kx][i][o] = scale *
    w[o][i][2-ky][2-kx]: tap (ky, kx) of the transposed conv's adjoint on the t grid, g_x[m,n] = sum W[ky,kx] g_t[2m+ky, 2n+kx]."""
    if dtype != BF16:
        raise DgeError("pack_up_dgrad_stream: bf16 only")
    cout, cin = w.shape[0], w.shape[1]
    return (w.detach().float() * float(scale)).flip(2, 3).permute(2, 3, 1, 0).reshape(9, cin, cout).to(torch.bfloat16).contiguous()


def up_dgrad_stream(g_z, w_packed, d_in, out_scale, addend, stats, dot_src, prep=None):
    """g_z [B,2H,2W,Cout] (gradient w.r.t. the up layer's pre-activation; d_in [B,Cout] or None still to be applied) -> [B,H,W,Cin]:
    FIR^T, transposed-conv adjoint and the data-gradient epilogue of conv2d(in_s2d=True, out_scale=, addend=, stats=, dot_src=,
    prep=) in one streaming launch (dge_up_dgrad_stream).  stats: SlotStats(B, Cin) or a zeroed [B,Cin,2] tensor."""
    B, FH, FW, cout = g_z.shape
    H, W = FH // 2, FW // 2
    _, cin, _ = w_packed.shape
    dt = dtype_of(g_z)
    if dot_src is None or stats is None:
        raise DgeError("up_dgrad_stream: needs stats and dot_src")
    if not up_dgrad_stream_supported(B, H, W, cin, cout, dt):
        raise DgeError(f"up_dgrad_stream: unsupported launch {cin} <- {cout} channels, dtype {dt}")
    out = torch.empty((B, H, W, cin), dtype=g_z.dtype, device=g_z.device)
    st, nslot, finish = _stats_target(stats, B, H, W, 32, g_z.device)
    pgain, pn, pns, pnb, pst = (1.0, None, None, 1, None) if prep is None else _prep_values(prep, nslot)
    _launch(lib().dge_up_dgrad_stream,
            (_p(g_z), _p(w_packed), _p(out), _f32(d_in), _f32(out_scale), _p(addend), _p(dot_src), _f32(st), nslot,
             0 if prep is None else 1, pgain, _f32(pn), 0 if pnb == 1 else H * W, _f32(pns), _f32(pst), B, H, W, cin, cout, dt, _stream()),
            "dge_up_dgrad_stream", 9.0 * cin * cout * H * W * B, (B, H, W, 4 * cout, cin, 3, False, True),
            (g_z, out, addend, dot_src, w_packed))
    if finish is not None:
        finish()
    return out


# ------------------------------------------------------------------ data gradient of the low-resolution up layers in phase form
UP_DGRAD_SMALL_UNITS = ((0, 0), (0, 2), (2, 0), (2, 2), (0, 1), (2, 1), (1, 0), (1, 2), (1, 1))     # (ky, kx) of unit u (walk order)


def up_dgrad_small_supported(B, Hin, Win, cin, cout, dtype):
    """True when the data gradient of an up layer cin -> cout on the Hin x Win input grid runs in phase form on the low-resolution
    kernel (csrc/conv_small.hip, dge_up_dgrad_small): bf16, cout in {256, 512}, cin % 64 == 0, grid <= 32^2; not in deterministic mode
    (that mode keeps its launches, as with up_dgrad_stream)."""
    return (not is_deterministic()) and bool(lib().dge_up_dgrad_small_supported(int(B), int(Hin), int(Win), int(cout), int(cin), int(dtype)))


def pack_up_dgrad_small(w, dtype=BF16, scale=1.0):
    """w: [Cout,Cin,3,3] f32 (the forward layer's parameter) -> the 9 non-zero units of the phase-form adjoint, [9, Cin, Cout] in
    MFMA-fragment order: unit u = scale * w[:, :, 2-ky, 2-kx]^T with (ky, kx) = UP_DGRAD_SMALL_UNITS[u]."""
    if dtype != BF16:
        raise DgeError("pack_up_dgrad_small: bf16 only")
    return pack_conv_weight(w, PACK_UPT2D_UNITS | PACK_FRAG, dtype, scale)


def up_dgrad_small(z_t2d, w_packed, out_scale, addend, stats, dot_src, prep=None):
    """z_t2d = fir_t2d(g_z, d) [B,H+1,W+1,4*Cout] -> [B,H,W,Cin]: what conv2d(z_t2d, PACK_UPT2D_DGRAD weights, in_t2d=True, out_scale=,
    addend=, stats=, dot_src=, prep=) computes, as the 9 non-zero units on the low-resolution kernel (dge_up_dgrad_small).
    w_packed: pack_up_dgrad_small's copy; stats: SlotStats(B, Cin) or a zeroed [B,Cin,2] tensor."""
    B, H1, W1, C4 = z_t2d.shape
    H, W, cout = H1 - 1, W1 - 1, C4 // 4
    cin = w_packed.shape[1]
    dt = dtype_of(z_t2d)
    if not getattr(w_packed, "_dge_frag", False) or tuple(w_packed.shape) != (9, cin, cout) or w_packed.dtype != z_t2d.dtype:
        raise DgeError("up_dgrad_small: w_packed must be pack_up_dgrad_small's copy of this layer's weight")
    if (dot_src is None) != (stats is None):
        raise DgeError("up_dgrad_small: stats and dot_src come together")
    if not up_dgrad_small_supported(B, H, W, cin, cout, dt):
        raise DgeError(f"up_dgrad_small: unsupported launch {cin} <- {cout} channels on {H}x{W}, dtype {dt}")
    out = torch.empty((B, H, W, cin), dtype=z_t2d.dtype, device=z_t2d.device)
    d = ConvDesc()
    d.in_t2d, d.w_layout, d.ksize = 1, 1, 3
    d.x, d.w_packed, d.y, d.addend, d.dot_src = _p(z_t2d), _p(w_packed), _p(out), _p(addend), _p(dot_src)
    d.out_scale = _f32(out_scale)
    st, nslot, finish = _stats_target(stats, B, H, W, 16, z_t2d.device)
    d.stats, d.stats_slots = _f32(st), nslot
    d.B, d.H, d.W, d.Cin, d.Cout = B, H, W, C4, cin
    nxt = _PREFETCH.link(_stream().value or 0, w_packed)
    if nxt is not None:
        d.prefetch_w, d.prefetch_ntot, d.prefetch_cin = C.c_void_p(nxt[0]), int(nxt[1]), int(nxt[2])
    if prep is not None:
        if stats is None:
            raise DgeError("up_dgrad_small: prep needs stats and dot_src")
        _set_prep(d, prep, nslot)
    d.noise_batch, d.act, d.bias_scale, d.gain, d.add_scale, d.dtype = 1, ACT_NONE, 1.0, 1.0, 1.0, dt
    _launch(lib().dge_up_dgrad_small, (C.byref(d), _stream()), "dge_up_dgrad_small", 9.0 * cin * cout * H * W * B,
            (B, H, W, C4, cin, 3, False, True), (z_t2d, out, addend, dot_src, w_packed), log=True)
    if finish is not None:
        finish()
    return out


# ------------------------------------------------------------------ inversion loop (embedding_v2.py)
TRACK_ARM_AT, TRACK_ARM_AFTER = 0, 1        # include/dge_hip.h DGE_TRACK_ARM_*


def latent_pnorm(w, p=2, out=None, out_l2=None):
    """||w||_p over the whole tensor (Tensor.norm(p), integer p >= 1) -> device scalar []; `out_l2` (optional [] / [1] f32) also
    receives ||w||_2.  Deterministic: one workgroup, fixed-order reduction."""
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=w.device)
    check(lib().dge_latent_pnorm_fwd(_f32(w.contiguous()), _p(out), _f32(out_l2), w.numel(), int(p), _stream()), "dge_latent_pnorm_fwd")
    return out


def latent_l2(w, out=None):
    """||w||_2 only -> device scalar []."""
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=w.device)
    check(lib().dge_latent_pnorm_fwd(_f32(w.contiguous()), None, _p(out), w.numel(), 2, _stream()), "dge_latent_pnorm_fwd")
    return out


def latent_pnorm_bwd(w, norm, g, p=2, beta=1.0, gout=None):
    """g += beta * gout * d||w||_p/dw (in place; g f32 contiguous, shape of w); 0 where the norm is 0."""
    check(lib().dge_latent_pnorm_bwd(_f32(w.contiguous()), _f32(norm), _f32(gout), _f32(g), w.numel(), int(p), float(beta), _stream()),
          "dge_latent_pnorm_bwd")
    return g


def wplus_lerp(w, avg, psi, out=None):
    """w [B,L,D]; avg [D] or [L,D] -> avg + psi*(w - avg) [B,L,D]"""
    B, L, D = w.shape
    if out is None:
        out = torch.empty((B, L, D), dtype=torch.float32, device=w.device)
    stride = D if avg.numel() == L * D else 0
    check(lib().dge_wplus_lerp(_f32(w.contiguous()), _f32(avg.contiguous()), stride, float(psi), _p(out), B, L, D, _stream()),
          "dge_wplus_lerp")
    return out


def wplus_lerp_bwd(g, psi, out=None, accumulate=False):
    """-> psi*g (accumulate: out += psi*g)"""
    g = g.float().contiguous()
    if out is None:
        out = torch.empty_like(g)
    check(lib().dge_wplus_lerp_bwd(_p(g), float(psi), _f32(out), g.numel(), 1 if accumulate else 0, _stream()), "dge_wplus_lerp_bwd")
    return out


def embed_track(loss, norm, w, istate, fstate, best_loss_w, best_norm_w, events, arm_rule, arm_iter, loss_hyst, norm_hyst):
    """One tracker update (include/dge_hip.h dge_embed_track): device scalars in, device state updated; no host sync."""
    if istate.dtype != torch.int32:
        raise DgeError("embed_track: istate must be int32")
    cap = events.shape[0]
    check(lib().dge_embed_track(_f32(loss), _f32(norm), _f32(w.contiguous()), w.numel(), _p(istate), _f32(fstate), _f32(best_loss_w),
                                _f32(best_norm_w), _f32(events), int(cap), int(arm_rule), int(arm_iter), float(loss_hyst),
                                float(norm_hyst), _stream()), "dge_embed_track")


# ---- a row per sample (LatentEmbedStep(independent=True)): row b is computed and tracked as the calls above do on w[b] alone
def latent_pnorm_rows(w, p=2, out=None, out_l2=None):
    """||w[b]||_p for every row of w [B, ...] -> [B]; `out_l2` (optional [B] f32) also receives ||w[b]||_2.  One workgroup per row,
    fixed-order reduction."""
    B = w.shape[0]
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=w.device)
    check(lib().dge_latent_pnorm_rows_fwd(_f32(w.contiguous()), _p(out), _f32(out_l2), B, w.numel() // B, int(p), _stream()),
          "dge_latent_pnorm_rows_fwd")
    log_kernel()
    return out


def latent_l2_rows(w, out=None):
    """||w[b]||_2 only -> [B]."""
    B = w.shape[0]
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=w.device)
    check(lib().dge_latent_pnorm_rows_fwd(_f32(w.contiguous()), None, _p(out), B, w.numel() // B, 2, _stream()), "dge_latent_pnorm_rows_fwd")
    log_kernel()
    return out


def latent_pnorm_rows_bwd(w, norm, g, p=2, beta=1.0, gout=None):
    """g[b] += beta * gout[b] * d||w[b]||_p/dw[b] (in place; g f32 contiguous, shape of w; norm, gout [B]); a row whose norm is 0 gets 0."""
    B = w.shape[0]
    check(lib().dge_latent_pnorm_rows_bwd(_f32(w.contiguous()), _f32(norm), _f32(gout), _f32(g), B, w.numel() // B, int(p), float(beta),
                                          _stream()), "dge_latent_pnorm_rows_bwd")
    log_kernel()
    return g


def embed_track_rows(loss, norm, w, istate, fstate, best_loss_w, best_norm_w, events, arm_rule, arm_iter, loss_hyst, norm_hyst):
    """One update of B trackers (include/dge_hip.h dge_embed_track_rows): loss, norm [B], w [B, ...], istate [B,4] int32, fstate [B,2],
    events [B,cap,4], best_* of w's shape; no host sync."""
    if istate.dtype != torch.int32:
        raise DgeError("embed_track_rows: istate must be int32")
    B = w.shape[0]
    if tuple(istate.shape) != (B, 4) or tuple(fstate.shape) != (B, 2) or events.shape[0] != B or loss.numel() != B or norm.numel() != B:
        raise DgeError("embed_track_rows: state shapes do not match the batch")
    for t in (loss, norm, istate, fstate, best_loss_w, best_norm_w, events):
        if not t.is_contiguous():
            raise DgeError("embed_track_rows: arguments must be contiguous")
    check(lib().dge_embed_track_rows(_f32(loss), _f32(norm), _f32(w.contiguous()), B, w.numel() // B, _p(istate), _f32(fstate),
                                     _f32(best_loss_w), _f32(best_norm_w), _f32(events), int(events.shape[1]), int(arm_rule),
                                     int(arm_iter), float(loss_hyst), float(norm_hyst), _stream()), "dge_embed_track_rows")
    log_kernel()



# ---- evaluation metrics on 8-bit images (include/dge_hip.h dge_quantize_u8 / dge_image_metrics_u8)
def quantize_u8(x, out=None):
    """x [B,C,H,W] f32 or bf16 in [-1,1] -> [B,H,W,C] uint8: the bytes save_image writes (x*0.5+0.5, clamp, *255+0.5, truncate)."""
    if x.dim() != 4:
        raise DgeError("quantize_u8: expected [B,C,H,W]")
    B, Cc, H, W = x.shape
    if out is None:
        out = torch.empty((B, H, W, Cc), dtype=torch.uint8, device=x.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W, Cc):
        raise DgeError("quantize_u8: out must be uint8 [B,H,W,C]")
    check(lib().dge_quantize_u8(_p(x), dtype_of(x), _p(out), B, Cc, H, W, _stream()), "dge_quantize_u8")
    log_kernel()
    return out


def image_metrics_u8_work_bytes(B, H, W):
    """Bytes of the `work` buffer of image_metrics_u8 (raises for the sizes the launch refuses)."""
    n = lib().dge_image_metrics_u8_work_bytes(int(B), int(H), int(W))
    if n < 0:
        check(n, "dge_image_metrics_u8_work_bytes")
    return n


def image_metrics_u8(a, b, work=None, isums=None, ssim=None, out=None):
    """a, b [B,H,W,3] uint8 contiguous -> (isums [B,5] int64, ssim [B] f64, out [B,4] f64 = psnr, ssim, mse, cosine), every image
    pair on its own.  No host sync; the buffers may be passed in (a captured graph reuses them), none has to be zeroed."""
    for t in (a, b):
        if t.dtype != torch.uint8:
            raise DgeError(f"image_metrics_u8: expected uint8 images, got {t.dtype}")
    if a.dim() != 4 or a.shape[3] != 3 or a.shape != b.shape:
        raise DgeError(f"image_metrics_u8: expected two [B,H,W,3] images of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    B, H, W, _ = a.shape
    nbytes = image_metrics_u8_work_bytes(B, H, W)
    dev = a.device
    if work is None:
        work = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    elif work.numel() * work.element_size() < nbytes:
        raise DgeError(f"image_metrics_u8: work holds {work.numel() * work.element_size()} bytes, {nbytes} needed")
    isums = torch.empty((B, 5), dtype=torch.int64, device=dev) if isums is None else isums
    ssim = torch.empty(B, dtype=torch.float64, device=dev) if ssim is None else ssim
    out = torch.empty((B, 4), dtype=torch.float64, device=dev) if out is None else out
    if isums.dtype != torch.int64 or ssim.dtype != torch.float64 or out.dtype != torch.float64 \
            or isums.numel() != 5 * B or ssim.numel() != B or out.numel() != 4 * B:
        raise DgeError("image_metrics_u8: isums int64 [B,5], ssim float64 [B], out float64 [B,4]")
    check(lib().dge_image_metrics_u8(_p(a), _p(b), B, H, W, _p(work), _p(isums), _p(ssim), _p(out), _stream()), "dge_image_metrics_u8")
    log_kernel()
    return isums, ssim, out


# ---- StyleGAN2 noise maps as free variables (include/dge_hip.h dge_s2_noise_grad / dge_noise_reg / dge_noise_normalize)
def s2_noise_grad(g, x=None, gain=1.0, ns=None, out=None, accumulate=False):
    """out [Bn, HW] f32 (Bn 1: a map shared by the batch, or B) (+)= ns * sum_c g_z[b, p, c] (shared: and over b, ascending).
    g NHWC [B,H,W,C] in the compute dtype: g_z when `x` is None (form A), else the gradient w.r.t. the layer output x, and the
    kernel applies gain * lrelu'(x) (form B).  ns: the layer's noise strength, a device f32 scalar."""
    B, H, W, Cc = g.shape
    if x is not None and (x.shape != g.shape or x.dtype != g.dtype):
        raise DgeError(f"s2_noise_grad: x {tuple(x.shape)} {x.dtype} does not match g {tuple(g.shape)} {g.dtype}")
    if ns is None or ns.numel() != 1:
        raise DgeError("s2_noise_grad: ns must be a device scalar")
    if out is None:
        if accumulate:
            raise DgeError("s2_noise_grad: accumulate needs out")
        out = torch.empty((1, H * W), dtype=torch.float32, device=g.device)
    Bn = out.numel() // (H * W)
    if out.numel() != Bn * H * W or Bn not in (1, B):
        raise DgeError(f"s2_noise_grad: out holds {out.numel()} floats, {H * W} (shared map) or {B * H * W} (a map per row) expected")
    check(lib().dge_s2_noise_grad(_p(g), _p(x), _f32(ns), _f32(out), B, Bn, H * W, Cc, float(gain), 1 if accumulate else 0, dtype_of(g),
                                  _stream()), "dge_s2_noise_grad")
    _log_dense("dge_s2_noise_grad")
    return out


NOISE_CHUNK = 1024          # elements of a chunk job (csrc/s2_noise_kernels.hip kChunk)


def noise_levels(R):
    """Levels of the regulariser's pyramid for a map of side R: the last one is the first of side <= 8."""
    n = 1
    while (R >> (n - 1)) > 8:
        n += 1
    return n


class NoiseTable:
    """The static layout of a set of square noise maps for dge_noise_reg / dge_noise_normalize, built once: the maps live in one
    flat f32 buffer, map m as [Bn, R_m, R_m] from float `offsets[m]` on (`view(flat, m)`); the device tables (map and job records)
    and the workspace belong to the table, so a captured iteration keeps their addresses."""

    def __init__(self, res, Bn, device):
        import numpy as np
        from ._lib import NoisePlan
        res = [int(r) for r in res]
        if not 1 <= len(res) <= 32 or Bn < 1:
            raise DgeError("NoiseTable: 1..32 maps, at least one row")
        for R in res:
            if R < 4 or R > 1024 or R & (R - 1):
                raise DgeError(f"NoiseTable: map side {R} (a power of two, 4..1024)")
        self.res, self.Bn, self.device = res, int(Bn), torch.device(device)
        map_dt = np.dtype([("off", "<i8"), ("work_off", "<i8"), ("R", "<i4"), ("nlev", "<i4"), ("pair0", "<i4"), ("cslot0", "<i4")])
        assert map_dt.itemsize == lib().dge_noise_map_size() and lib().dge_noise_job_size() == 16
        maps = np.zeros(len(res), dtype=map_dt)
        pool0, pool1, mom, pairs, chunks = [], [], [], [], []
        off = lev = 0
        self.offsets = []
        for m, R in enumerate(res):
            nlev = noise_levels(R)
            maps[m] = (off, lev, R, nlev, len(pairs), len(chunks))
            self.offsets.append(off)
            off += Bn * R * R
            lev += Bn * sum((R >> l) ** 2 for l in range(1, nlev))
            for src, jobs in ((0, pool0), (5, pool1)):
                if nlev - 1 > src:
                    t = max(1, (R >> src) // 32)
                    jobs += [(m, src, ty, tx) for ty in range(t) for tx in range(t)]
            for l in range(nlev):
                nch = -(-((R >> l) ** 2) // NOISE_CHUNK)
                pairs.append((m, l, len(mom), nch))
                mom += [(m, l, c, len(mom) + c) for c in range(nch)]
            nch = -(-(R * R) // NOISE_CHUNK)
            chunks += [(m, 0, c, len(chunks) + c) for c in range(nch)]
        if len(pairs) > 256:
            raise DgeError("NoiseTable: more than 256 (map, level) pairs")
        jobs = np.array(pool0 + pool1 + mom + pairs + chunks, dtype=np.int32).reshape(-1, 4)
        self.numel = off
        self._maps = torch.from_numpy(maps.view(np.uint8).copy()).to(self.device)
        self._jobs = torch.from_numpy(jobs.copy()).to(self.device)
        self.device = self._maps.device          # (with its index: what a tensor on it reports)
        self.plan = NoisePlan(self._maps.data_ptr(), self._jobs.data_ptr(), len(res), self.Bn, len(pool0), len(pool1), len(mom), len(pairs),
                              len(chunks), 0, off, lev)
        nb = max(lib().dge_noise_reg_work_bytes(C.byref(self.plan)), lib().dge_noise_normalize_work_bytes(C.byref(self.plan)))
        if nb < 0:
            check(nb, "dge_noise_reg_work_bytes")
        self.work = torch.empty((nb + 3) // 4, dtype=torch.float32, device=self.device)

    def view(self, flat, m):
        R = self.res[m]
        return flat[self.offsets[m]:self.offsets[m] + self.Bn * R * R].view(self.Bn, R, R)

    def _flat(self, t, what):
        if t.dtype != torch.float32 or t.numel() != self.numel or t.device != self.device:
            raise DgeError(f"{what}: expected the table's flat f32 buffer of {self.numel} floats on {self.device}")
        return _f32(t)


def noise_reg(table, flat, grad=None, scale=1.0, accumulate=False, out=None):
    """reg [Bn] of the maps in `flat` (NoiseTable layout); with `grad` (same layout): grad (+)= scale * d reg[b] / d flat."""
    if out is None:
        out = torch.empty(table.Bn, dtype=torch.float32, device=table.device)
    if out.numel() != table.Bn:
        raise DgeError("noise_reg: out holds one value per row")
    check(lib().dge_noise_reg(C.byref(table.plan), table._flat(flat, "noise_reg"), _f32(out),
                              None if grad is None else table._flat(grad, "noise_reg"), float(scale), 1 if accumulate else 0,
                              _p(table.work), table.work.numel() * 4, _stream()), "dge_noise_reg")
    _log_dense("dge_noise_reg")
    return out


def noise_normalize(table, flat):
    """Every row of every map of `flat` to zero mean and unit mean square, in place."""
    check(lib().dge_noise_normalize(C.byref(table.plan), table._flat(flat, "noise_normalize"), _p(table.work), table.work.numel() * 4,
                                    _stream()), "dge_noise_normalize")
    _log_dense("dge_noise_normalize")
    return flat


# ---- StyleGAN2's projector (include/dge_hip.h dge_adam_multi / dge_w_broadcast / dge_rows_mean_std / dge_area_pool_bwd)
def _host_or_dev(v, what):
    """(host float, device pointer or None) of a scalar given as a Python number or as a one-element f32 device tensor"""
    if torch.is_tensor(v):
        if v.numel() != 1:
            raise DgeError(f"{what}: a device scalar holds one float")
        return 0.0, _f32(v)
    return float(v), None


def adam_multi(params, grads, exp_avg, exp_avg_sq, beta1, beta2, eps, step=0.0, inv_sqrt_bc2=1.0, scalars=None):
    """One torch.optim.Adam update of every tensor of the lists, in one launch (in place on params, exp_avg, exp_avg_sq).
    step = lr / (1 - beta1^t), inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t); `scalars`: a [2] f32 device tensor holding the two instead."""
    n = len(params)
    if not (len(grads) == len(exp_avg) == len(exp_avg_sq) == n):
        raise DgeError("adam_multi: the four lists hold one tensor per parameter")
    for quad in zip(params, grads, exp_avg, exp_avg_sq):
        if len({t.numel() for t in quad}) != 1:
            raise DgeError("adam_multi: a parameter, its gradient and its moments have one size")
    if scalars is not None and scalars.numel() != 2:
        raise DgeError("adam_multi: scalars holds two floats (step, 1/sqrt(bc2))")
    VP = C.c_void_p * n
    ptrs = [VP(*[_f32(t).value for t in ts]) for ts in (params, grads, exp_avg, exp_avg_sq)]
    check(lib().dge_adam_multi(n, *ptrs, (C.c_long * n)(*[p.numel() for p in params]), float(beta1), float(beta2), float(eps), float(step),
                               float(inv_sqrt_bc2), _f32(scalars), _stream()), "dge_adam_multi")
    log_kernel()


def w_broadcast(w, L, noise=None, scale=0.0, out=None):
    """w [B,D], noise [B,D] or None -> ws [B,L,D] = (w + noise * scale) in every row l; `scale`: a number or a device scalar."""
    B, D = w.shape
    if noise is not None and tuple(noise.shape) != (B, D):
        raise DgeError(f"w_broadcast: noise must have w's shape {(B, D)}, got {tuple(noise.shape)}")
    if out is None:
        out = torch.empty((B, L, D), dtype=torch.float32, device=w.device)
    elif tuple(out.shape) != (B, L, D):
        raise DgeError(f"w_broadcast: out must be {(B, L, D)}")
    sc, sd = _host_or_dev(scale, "w_broadcast")
    check(lib().dge_w_broadcast(_f32(w), _f32(noise), sc, sd, _f32(out), B, int(L), D, _stream()), "dge_w_broadcast")
    log_kernel()
    return out


def w_broadcast_bwd(g_ws, out=None):
    """g_ws [B,L,D] -> g_w [B,D], the sum over l in ascending order."""
    B, L, D = g_ws.shape
    if out is None:
        out = torch.empty((B, D), dtype=torch.float32, device=g_ws.device)
    check(lib().dge_w_broadcast_bwd(_f32(g_ws), _f32(out), B, L, D, _stream()), "dge_w_broadcast_bwd")
    log_kernel()
    return out


def rows_mean_std(x):
    """x [N,D] f32 -> (mean [D] over the rows, std [1] = sqrt(sum (x - mean)^2 / N)): the projector's w_avg and w_std."""
    N, D = x.shape
    nb = lib().dge_rows_mean_std_work_bytes(N, D)
    if nb < 0:
        check(nb, "dge_rows_mean_std_work_bytes")
    work = torch.empty((nb + 3) // 4, dtype=torch.float32, device=x.device)
    mean = torch.empty(D, dtype=torch.float32, device=x.device)
    std = torch.empty(1, dtype=torch.float32, device=x.device)
    check(lib().dge_rows_mean_std(_f32(x), N, D, _p(mean), _p(std), _p(work), work.numel() * 4, _stream()), "dge_rows_mean_std")
    log_kernel()
    return mean, std


def cols_mean_std(x):
    """x [N,D] f32 -> (mean [D], std [D]) over the rows, std = sqrt(sum (x - mean)^2 / N) per column (dge_cols_mean_std)."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise DgeError("cols_mean_std: x is a contiguous float32 matrix [N,D]")
    N, D = x.shape
    nb = lib().dge_cols_mean_std_work_bytes(N, D)
    if nb < 0:
        check(nb, "dge_cols_mean_std_work_bytes")
    work = torch.empty((nb + 3) // 4, dtype=torch.float32, device=x.device)
    mean = torch.empty(D, dtype=torch.float32, device=x.device)
    std = torch.empty(D, dtype=torch.float32, device=x.device)
    check(lib().dge_cols_mean_std(_f32(x), N, D, _p(mean), _p(std), _p(work), work.numel() * 4, _stream()), "dge_cols_mean_std")
    log_kernel()
    return mean, std


# ---- dense linear algebra of the semantic directions (include/dge_hip.h dge_gram / dge_eigh_sym)
def gram(x, mean=None, row_norm=False, scale=1.0):
    """x [N,D] f32 (rows may be strided: a column slice of a wider matrix) -> out [D,D] = scale * sum_n u_n u_n^T with u_n = x_n / |x_n|
    (row_norm), x_n - mean (mean [D]) or x_n; out == out^T to the bit (dge_gram)."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or (x.shape[1] > 1 and x.stride(1) != 1):
        raise DgeError("gram: x is a float32 device matrix [N,D] whose rows are contiguous")
    N, D = x.shape
    ldx = x.stride(0) if N > 1 else max(x.stride(0), D)
    if mean is not None and (mean.numel() != D or not mean.is_cuda):
        raise DgeError(f"gram: mean holds D = {D} device floats")
    nb = lib().dge_gram_work_bytes(N, D)
    if nb < 0:
        check(nb, "dge_gram_work_bytes")
    work = torch.empty((nb + 3) // 4, dtype=torch.float32, device=x.device)
    out = torch.empty((D, D), dtype=torch.float32, device=x.device)
    check(lib().dge_gram(C.c_void_p(x.data_ptr()), N, D, ldx, _f32(mean), 1 if row_norm else 0, float(scale), _p(out), _p(work),
                         work.numel() * 4, _stream()), "dge_gram")
    log_kernel()
    return out


def eigh_sym(a, max_sweeps=30):
    """a [D,D] f32, symmetric (the upper triangle is read) -> (evals [D] descending, evecs [D,D] with the unit eigenvector of
    evals[k] in row k, its largest component positive, (sweeps, off(A))) (dge_eigh_sym).  One host read per sweep.  Not converged
    after max_sweeps: DgeError, whose `partial` attribute holds the same triple of the last iterate."""
    if a.dim() != 2 or a.shape[0] != a.shape[1]:
        raise DgeError(f"eigh_sym: a is a square matrix, got {tuple(a.shape)}")
    D = a.shape[0]
    nb = lib().dge_eigh_sym_work_bytes(D)
    if nb < 0:
        check(nb, "dge_eigh_sym_work_bytes")
    work = torch.empty((nb + 7) // 8, dtype=torch.float64, device=a.device)
    evals = torch.empty(D, dtype=torch.float32, device=a.device)
    evecs = torch.empty((D, D), dtype=torch.float32, device=a.device)
    status = (C.c_double * 2)(0.0, 0.0)
    rc = lib().dge_eigh_sym(_f32(a), D, _p(evals), _p(evecs), status, _p(work), work.numel() * 8, int(max_sweeps), _stream())
    result = evals, evecs, (int(status[0]), float(status[1]))
    if rc == -2:
        err = DgeError(f"dge_eigh_sym failed ({rc}): {lib().dge_last_error().decode()}")
        err.partial = result
        raise err
    check(rc, "dge_eigh_sym")
    log_kernel()
    return result


def area_pool_bwd(g_pooled, k, out=None):
    """g_pooled [B,C,h,w] f32 -> [B,C,h*k,w*k]: the adjoint of the k x k area pooling (each value / k^2 to its k x k pixels)."""
    B, Cc, h, w = g_pooled.shape
    if out is None:
        out = torch.empty((B, Cc, h * k, w * k), dtype=torch.float32, device=g_pooled.device)
    check(lib().dge_area_pool_bwd(_f32(g_pooled), _f32(out), B * Cc, h * k, w * k, int(k), _stream()), "dge_area_pool_bwd")
    log_kernel()
    return out


def area_pool(x, k):
    """x [B,C,H,W] f32 -> the k x k area means [B,C,H/k,W/k] (dge_crop_pool_multi on the whole image)."""
    B, Cc, H, W = x.shape
    out = torch.empty((B, Cc, H // k, W // k), dtype=torch.float32, device=x.device)
    check(lib().dge_crop_pool_multi((C.c_void_p * 1)(_f32(x).value), (C.c_void_p * 1)(_p(out).value), (C.c_int * 4)(0, 0, H, W),
                                    (C.c_int * 1)(int(k)), 1, B * Cc, H, W, _stream()), "dge_crop_pool_multi")
    _log_dense("dge_crop_pool_multi")
    return out


def randn_seeded(out, seeds, seeds_dev=None):
    """Row r of out [R,D] <- the first D normals of draw 0 under seed seeds[r] (dge_randn, a launch per row: the Philox key is the
    seed).  seeds_dev: an int64 device tensor [R] read in place of `seeds` (a captured iteration is replayed with new seeds).
    Every launch is named in KERNEL_LOG (the entry point's name: it selects no kernel instantiation)."""
    R, D = out.shape
    LL, ULL, UI = C.c_longlong * 1, C.c_ulonglong * 1, C.c_uint * 1
    for r in range(R):
        sd = C.c_void_p(seeds_dev.data_ptr() + 8 * r) if seeds_dev is not None else None
        check(lib().dge_randn(C.c_void_p(_f32(out).value + 4 * r * D), 1, LL(0), LL(D), ULL(0), UI(0),
                              C.c_ulonglong(int(seeds[r]) & 0xFFFFFFFFFFFFFFFF), sd, _stream()), "dge_randn")
        _log_dense("dge_randn")
    return out


# ---- masked LPIPS (include/dge_hip.h dge_mask_pyramid / dge_lpips_prep_masked / dge_lpips_head_w / dge_mask_blend)
MASK_LEVELS = 5


def mask_level_shapes(H, W):
    """(h_k, w_k) of the five mask levels: floor halving, the grids of the five LPIPS-VGG taps."""
    return [(H >> k, W >> k) for k in range(MASK_LEVELS)]


def mask_pyramid_work_bytes(B, H, W):
    n = lib().dge_mask_pyramid_work_bytes(int(B), int(H), int(W))
    if n < 0:
        check(n, "dge_mask_pyramid_work_bytes")
    return n


def mask_pyramid(m, levels=None, inv_sum=None, sums=None, work=None):
    """m [B,H,W] f32 -> (levels: the list of the five levels [B,h_k,w_k], views of one flat buffer; inv_sum [B,5] = 1 / sum of a
    level, 0 where the sum is 0; sums [B,5]).  `levels` (the flat buffer), inv_sum, sums and work may be passed in to be refilled in
    place (a captured iteration keeps reading them).  No host sync."""
    if m.dim() != 3 or m.dtype != torch.float32:
        raise DgeError(f"mask_pyramid: expected a [B,H,W] f32 mask, got {tuple(m.shape)} {m.dtype}")
    B, H, W = m.shape
    shapes = mask_level_shapes(H, W)
    total = B * sum(h * w for h, w in shapes)
    dev = m.device
    flat = torch.empty(total, dtype=torch.float32, device=dev) if levels is None else levels
    if flat.dtype != torch.float32 or flat.numel() != total:
        raise DgeError(f"mask_pyramid: levels must be a flat f32 buffer of {total} floats")
    inv_sum = torch.empty((B, MASK_LEVELS), dtype=torch.float32, device=dev) if inv_sum is None else inv_sum
    sums = torch.empty((B, MASK_LEVELS), dtype=torch.float32, device=dev) if sums is None else sums
    if inv_sum.numel() != B * MASK_LEVELS or sums.numel() != B * MASK_LEVELS:
        raise DgeError("mask_pyramid: inv_sum and sums hold [B,5] floats")
    nb = mask_pyramid_work_bytes(B, H, W)
    if work is None:
        work = torch.empty(nb // 4, dtype=torch.float32, device=dev)
    check(lib().dge_mask_pyramid(_f32(m.contiguous()), _f32(flat), _f32(inv_sum), _f32(sums), B, H, W, _p(work),
                                 work.numel() * work.element_size(), _stream()), "dge_mask_pyramid")
    _log_dense("dge_mask_pyramid")
    views, off = [], 0
    for h, w in shapes:
        views.append(flat[off:off + B * h * w].view(B, h, w))
        off += B * h * w
    return views, inv_sum, sums


def lpips_prep_masked(img, mask, x, shift3, scale3, cpad):
    """x [B,h,w,cpad] <- ((mask * img) - shift) / scale, NHWC (dge_lpips_prep with the per-pixel factor mask [B,h,w])."""
    B, _, h, w = img.shape
    if mask.dtype != torch.float32 or mask.numel() != B * h * w:
        raise DgeError(f"lpips_prep_masked: the mask holds {mask.numel()} floats, {B * h * w} expected")
    check(lib().dge_lpips_prep_masked(_f32(img), _f32(mask), _p(x), B, h * w, int(cpad), shift3, scale3, dtype_of(x), _stream()),
          "dge_lpips_prep_masked")
    _log_dense("dge_lpips_prep_masked")
    return x


def lpips_prep_bwd_masked(gx, mask, gimg, scale3, cpad, factor=1.0, accumulate=False):
    """gimg [B,3,h,w] (+)= (factor * gx[..., :3] / scale) * mask (dge_lpips_prep_bwd with the per-pixel factor mask [B,h,w])."""
    B, _, h, w = gimg.shape
    if mask.dtype != torch.float32 or mask.numel() != B * h * w:
        raise DgeError(f"lpips_prep_bwd_masked: the mask holds {mask.numel()} floats, {B * h * w} expected")
    check(lib().dge_lpips_prep_bwd_masked(_p(gx), _f32(mask), _f32(gimg), B, h * w, int(cpad), scale3, float(factor), 1 if accumulate else 0,
                                          dtype_of(gx), _stream()), "dge_lpips_prep_bwd_masked")
    _log_dense("dge_lpips_prep_bwd_masked")
    return gimg


def lpips_head_w_slots(HW, Cc, dtype):
    """Slots per row of one tap's weighted head (the workgroups that walk a row's pixels)."""
    n = lib().dge_lpips_head_w_slots(int(HW), int(Cc), int(dtype))
    if n < 0:
        check(n, "dge_lpips_head_w_slots")
    return n


def lpips_head_w(feat, lin, mk, inv_sum, tap, slots, g1=None, gscale=1.0):
    """The weighted head of tap `tap`: feat [2B,h,w,C], mk [B,h,w], inv_sum [B,5]; slots [B, lpips_head_w_slots] is written, g1
    (optional, [B,h,w,C]) = gscale * mk * inv_sum[:, tap] * d d / d feat[B:]."""
    B2, h, w, Cc = feat.shape
    B = B2 // 2
    dt = dtype_of(feat)
    n = lpips_head_w_slots(h * w, Cc, dt)
    if mk.numel() != B * h * w or inv_sum.numel() != B * MASK_LEVELS or slots.numel() != B * n:
        raise DgeError(f"lpips_head_w: mk holds {mk.numel()} floats ({B * h * w} expected), slots {slots.numel()} ({B * n} expected)")
    if g1 is not None and (g1.dtype != feat.dtype or g1.numel() != B * h * w * Cc):
        raise DgeError("lpips_head_w: g1 must be [B,h,w,C] in the features' dtype")
    check(lib().dge_lpips_head_w(_p(feat), _f32(lin), _f32(mk), _f32(inv_sum), int(tap), _f32(slots), _p(g1), B, h * w, Cc, float(gscale), dt,
                                 _stream()), "dge_lpips_head_w")
    _log_dense("dge_lpips_head_w")
    return g1


def lpips_head_w_finalize(slots, offsets, nslots, inv_sum, dist):
    """dist [B] <- sum over the five taps of inv_sum[b,k] * (the slots of tap k, row b, in a fixed order).  slots: the flat
    workspace; offsets[k], nslots[k]: where tap k's [B, nslots[k]] block starts and how many slots a row has."""
    B = dist.numel()
    if len(offsets) != MASK_LEVELS or len(nslots) != MASK_LEVELS or offsets[-1] + B * nslots[-1] > slots.numel():
        raise DgeError("lpips_head_w_finalize: five tap blocks inside the workspace")
    check(lib().dge_lpips_head_w_finalize(_f32(slots), (C.c_longlong * MASK_LEVELS)(*[int(o) for o in offsets]),
                                          (C.c_int * MASK_LEVELS)(*[int(n) for n in nslots]), _f32(inv_sum), _f32(dist), B, _stream()),
          "dge_lpips_head_w_finalize")
    _log_dense("dge_lpips_head_w_finalize")
    return dist


def mask_blend(m, a, b, out=None):
    """m [B,1,H,W], a, b [B,3,H,W] f32 -> m * a + (1 - m) * b, the bits of torch's expression (feeds quantize_u8)."""
    B, Cc, H, W = a.shape
    if Cc != 3 or a.shape != b.shape or m.numel() != B * H * W or any(t.dtype != torch.float32 for t in (m, a, b)):
        raise DgeError(f"mask_blend: two [B,3,H,W] f32 images and a [B,1,H,W] f32 mask, got {tuple(a.shape)}, {tuple(b.shape)}, {tuple(m.shape)}")
    if out is None:
        out = torch.empty_like(a, memory_format=torch.contiguous_format)
    check(lib().dge_mask_blend(_f32(m.contiguous()), _f32(a.contiguous()), _f32(b.contiguous()), _f32(out), B, H * W, _stream()), "dge_mask_blend")
    _log_dense("dge_mask_blend")
    return out


# ---- region directions (include/dge_hip.h dge_gram_cols / dge_fd_pool_diff / dge_wp_axis_pairs / dge_matmul_f64acc)
def _matrix_view(t, what):
    """(rows, columns, row stride) of a float32 device matrix whose rows are contiguous (a row or column slice of a wider one)"""
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.shape[0] < 1 or t.shape[1] < 1 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise DgeError(f"{what}: a non-empty float32 device matrix whose rows are contiguous")
    R, Cn = t.shape
    return R, Cn, (t.stride(0) if R > 1 else max(t.stride(0), Cn))


def gram_cols_chunk(N):
    """the columns of one chunk of dge_gram_cols at N columns (one partial tile per chunk and tile, added in chunk order)"""
    c = lib().dge_gram_cols_chunk(int(N))
    if c < 0:
        check(int(c), "dge_gram_cols_chunk")
    return int(c)


def gram_cols(x, wgt=None, scale=1.0, both=None):
    """x [K,N] f32, K-major with contiguous rows (rows may be strided) -> out_a [K,K] = scale * sum_n w_n x_n x_n^T over the columns,
    w_n = wgt[n mod P] for wgt of P floats (P divides N); with a weight also out_b = scale * sum_n (1 - w_n) x_n x_n^T from the same
    read (both=False: out_a alone).  wgt=None: w = 1, one output.  Both are symmetric to the bit (dge_gram_cols).  Returns out_a or
    (out_a, out_b)."""
    K, N, ldx = _matrix_view(x, "gram_cols: x")
    both = wgt is not None if both is None else bool(both)
    if both and wgt is None:
        raise DgeError("gram_cols: the complement output needs a weight")
    P = 1
    if wgt is not None:
        if wgt.dtype != torch.float32 or not wgt.is_cuda or wgt.numel() < 1 or N % wgt.numel():
            raise DgeError(f"gram_cols: wgt holds P device floats with P dividing N = {N}")
        P = wgt.numel()
    nb = lib().dge_gram_cols_work_bytes(K, N)
    if nb < 0:
        check(int(nb), "dge_gram_cols_work_bytes")
    work = torch.empty(nb // 4, dtype=torch.float32, device=x.device)
    out_a = torch.empty((K, K), dtype=torch.float32, device=x.device)
    out_b = torch.empty((K, K), dtype=torch.float32, device=x.device) if both else None
    check(lib().dge_gram_cols(C.c_void_p(x.data_ptr()), K, N, ldx, _f32(wgt), P, float(scale), _p(out_a), _p(out_b), _p(work), nb, _stream()),
          "dge_gram_cols")
    log_kernel()
    return (out_a, out_b) if both else out_a


def fd_pool_diff(img, s, scale, x):
    """img [2n,C,H,W] f32 -> row j of x [n, >= C*(H/s)*(W/s)] (a row slice of the Jacobian operand) = scale * the s x s window sums of
    img[2j] - img[2j+1] (dge_fd_pool_diff)."""
    if img.dim() != 4 or img.shape[0] % 2 or img.shape[0] < 2:
        raise DgeError(f"fd_pool_diff: img holds an even number of images [2n,C,H,W], got {tuple(img.shape)}")
    B, Cc, H, W = img.shape
    n, _, ldx = _matrix_view(x, "fd_pool_diff: x")
    if n != B // 2 or int(s) < 1 or H % int(s) or W % int(s) or x.shape[1] != Cc * (H // int(s)) * (W // int(s)):
        raise DgeError(f"fd_pool_diff: x is {tuple(x.shape)} for {B // 2} image pairs of {Cc} x {H} x {W} pooled by {s}")
    check(lib().dge_fd_pool_diff(_f32(img), n, Cc, H, W, int(s), float(scale), C.c_void_p(x.data_ptr()), ldx, _stream()), "dge_fd_pool_diff")
    log_kernel()
    return x


def wp_axis_pairs(wp, q, r0, r1, h, out=None):
    """wp [L,D], q [n,D] (rows may be strided) -> out [2n,L,D]: code 2j = fma(h, q_j, wp), code 2j+1 = fma(-h, q_j, wp) on W+ rows
    r0 .. r1 - 1, bit copies of wp elsewhere (dge_wp_axis_pairs)."""
    if wp.dim() != 2:
        raise DgeError(f"wp_axis_pairs: wp is one code [L,D], got {tuple(wp.shape)}")
    L, D = wp.shape
    n, Dq, ldq = _matrix_view(q, "wp_axis_pairs: q")
    if Dq != D:
        raise DgeError(f"wp_axis_pairs: q has {Dq} columns, the code {D}")
    if out is None:
        out = torch.empty((2 * n, L, D), dtype=torch.float32, device=wp.device)
    elif tuple(out.shape) != (2 * n, L, D):
        raise DgeError(f"wp_axis_pairs: out must be {(2 * n, L, D)}")
    check(lib().dge_wp_axis_pairs(_f32(wp), C.c_void_p(q.data_ptr()), ldq, n, L, D, int(r0), int(r1), float(h), _f32(out), _stream()),
          "dge_wp_axis_pairs")
    log_kernel()
    return out


def matmul_f64acc(a, b, trans_b=False, out=None):
    """a [M,Kk] times b [Kk,N] (trans_b: b [N,Kk], its transpose taken) -> out [M,N], every dimension <= 1024: f32 operands, the
    products and the ascending-k sum in f64, rounded once (dge_matmul_f64acc).  Rows may be strided."""
    M, Kk, lda = _matrix_view(a, "matmul_f64acc: a")
    Rb, Cb, ldb = _matrix_view(b, "matmul_f64acc: b")
    N, Kb = (Rb, Cb) if trans_b else (Cb, Rb)
    if Kb != Kk:
        raise DgeError(f"matmul_f64acc: a is {tuple(a.shape)}, b {tuple(b.shape)}{' transposed' if trans_b else ''}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    Mo, No, ldo = _matrix_view(out, "matmul_f64acc: out")
    if (Mo, No) != (M, N):
        raise DgeError(f"matmul_f64acc: out must be {(M, N)}")
    check(lib().dge_matmul_f64acc(C.c_void_p(a.data_ptr()), lda, C.c_void_p(b.data_ptr()), ldb, 1 if trans_b else 0, C.c_void_p(out.data_ptr()),
                                  ldo, M, N, Kk, _stream()), "dge_matmul_f64acc")
    log_kernel()
    return out
