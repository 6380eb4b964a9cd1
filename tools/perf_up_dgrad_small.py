"""Data gradient of the low-resolution 512 -> 512 up layers (layers 1 / 3 / 5 / 7 of the 1024^2 generator, input grids 4^2 .. 32^2) with
the tail backward of the layer below in its epilogue: the phase form on the low-resolution kernel (ops.fir_t2d + ops.up_dgrad_small,
csrc/conv_small.hip) against the launch it replaces - the folded space-to-depth conv2d at 4^2 .. 16^2, ops.fir_t2d + conv2d(in_t2d)
at 32^2 - per layer, in one process, interleaved (dev tool, GPU box).  `hot`: 20 calls back to back (weights stay in cache); `cold`:
every call timed on its own after a 512 MB fill, which is how a training step finds the weights.
usage: perf_up_dgrad_small.py [B=8] [rounds=5]"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd
from dge_amd import ops, s2_conv
from dge_amd._lib import last_kernel


def timeit(f, n=20):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


FLUSH = None


def timeit_cold(f, n=20):
    global FLUSH
    if FLUSH is None:
        FLUSH = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    t = []
    for _ in range(n):
        FLUSH.fill_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3)
    return sorted(t)[n // 2]


B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
C = 512
s2_conv.UP_DG_SMALL = False                          # "old" is the route this launch replaced: conv2d in phase form or folded
g = torch.Generator(device="cuda").manual_seed(0)
gain = math.sqrt(2.0)
wscale = 1 / math.sqrt(9 * C)
print(f"B={B}, 512 <- 512 channels; us per call (fir_t2d and SlotStats allocation included), median [min .. max] of {rounds} interleaved rounds of 20")
for R in (4, 8, 16, 32):
    gz = torch.randn(B, 2 * R, 2 * R, C, device="cuda", generator=g).to(torch.bfloat16)
    x = torch.randn(B, R, R, C, device="cuda", generator=g).to(torch.bfloat16)
    add = torch.randn(B, R, R, C, device="cuda", generator=g).to(torch.bfloat16)
    d_in = 0.5 + torch.rand(B, C, device="cuda", generator=g)
    s = 1 + 0.3 * torch.randn(B, C, device="cuda", generator=g)
    noise = torch.randn(1, R, R, device="cuda", generator=g); ns = torch.tensor([0.3], device="cuda")
    w = torch.randn(C, C, 3, 3, device="cuda", generator=g)
    t2d = s2_conv.dgrad_route(s2_conv.LayerShape(True, 2 * R, C, C), B, ops.BF16, True, True).kind.endswith("t2d")
    pk = ops.pack_conv_weight(w, ops.PACK_UPT2D_DGRAD if t2d else ops.pack_mode_for(w, ops.PACK_UPFOLD_DGRAD, R, R, ops.BF16), ops.BF16, wscale)
    pu = ops.pack_up_dgrad_small(w, ops.BF16, wscale)
    names = {}

    def prep():
        return dict(gain=gain, noise=noise, ns=ns, stats=ops.SlotStats(B, C, "cuda"))

    def old():
        if t2d:
            ops.conv2d(ops.fir_t2d(gz, d_in), pk, C, 3, in_t2d=True, out_scale=s, addend=add, add_scale=1.0, stats=ops.SlotStats(B, C, "cuda"), dot_src=x, prep=prep())
        else:
            ops.conv2d(gz, pk, C, 3, in_s2d=True, in_scale=d_in, out_scale=s, addend=add, add_scale=1.0, stats=ops.SlotStats(B, C, "cuda"), dot_src=x, prep=prep())
        names["old"] = last_kernel()

    def new():
        ops.up_dgrad_small(ops.fir_t2d(gz, d_in), pu, s, add, ops.SlotStats(B, C, "cuda"), x, prep=prep())
        names["new"] = last_kernel()

    def fir():
        ops.fir_t2d(gz, d_in)

    cases = [("old", old), ("new", new), ("fir_t2d", fir)]
    res = {(k, m): [] for k, _ in cases for m in ("hot", "cold")}
    for _ in range(rounds):
        for k, f in cases:
            res[(k, "hot")].append(timeit(f))
            res[(k, "cold")].append(timeit_cold(f))
    for k, _ in cases:
        line = f"{R:3d}^2 {k:>8}"
        for m in ("hot", "cold"):
            v = sorted(res[(k, m)])
            line += f"  {m} {v[len(v) // 2]:7.1f} [{v[0]:7.1f} .. {v[-1]:7.1f}]"
        print(line + f"  {names.get(k, 'fir_t2d')}")
