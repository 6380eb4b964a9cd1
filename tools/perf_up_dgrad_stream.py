"""Data gradient of the 64 -> 32 up layer (layer 15 of the 1024^2 generator, 1024^2 -> 512^2): the streaming adjoint with the tail
backward of layer 14 in its epilogue (ops.up_dgrad_stream, csrc/upconv_stream_bwd.hip) against the pair it replaces - the folded
space-to-depth conv (conv_igemm mode 33) followed by dge_modconv_bwd_prep - in one process, interleaved (dev tool, GPU box).
usage: perf_up_dgrad_stream.py [B=8] [rounds=5]"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd
from dge_amd import ops
from dge_amd._lib import last_kernel


def timeit(f, n=20):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
R, cof, cif = 512, 32, 64
g = torch.Generator(device="cuda").manual_seed(0)
gain = math.sqrt(2.0)
gz = torch.randn(B, 2 * R, 2 * R, cof, device="cuda", generator=g).to(torch.bfloat16)
x = torch.randn(B, R, R, cif, device="cuda", generator=g).to(torch.bfloat16)
add = torch.randn(B, R, R, cif, device="cuda", generator=g).to(torch.bfloat16)
d_in = 0.5 + torch.rand(B, cof, device="cuda", generator=g)
d_prev = 0.5 + torch.rand(B, cif, device="cuda", generator=g)
s = 1 + 0.3 * torch.randn(B, cif, device="cuda", generator=g)
noise = torch.randn(1, R, R, device="cuda", generator=g); ns = torch.tensor([0.3], device="cuda")
w = torch.randn(cof, cif, 3, 3, device="cuda", generator=g)
wscale = 1 / math.sqrt(9 * cif)
pk = ops.pack_conv_weight(w, ops.pack_mode_for(w, ops.PACK_UPFOLD_DGRAD, R, R, ops.BF16), ops.BF16, wscale)
ps = ops.pack_up_dgrad_stream(w, ops.BF16, wscale)
Rr = torch.zeros(B, cif, 3, device="cuda")
holder, names = {}, {}


def old_conv():
    holder["g"] = ops.conv2d(gz, pk, cif, 3, in_s2d=True, in_scale=d_in, out_scale=s, addend=add, add_scale=1.0, stats=ops.SlotStats(B, cif, "cuda"), dot_src=x)
    names["old_conv"] = last_kernel()


def old_pass():
    ops.modconv_bwd_prep(holder["g"], x, d_prev, noise, gain, Rr)


def old_pair():
    old_conv(); old_pass()


def new_plain():
    ops.up_dgrad_stream(gz, ps, d_in, s, add, ops.SlotStats(B, cif, "cuda"), x)
    names["new_plain"] = last_kernel()


def new_prep():
    ops.up_dgrad_stream(gz, ps, d_in, s, add, ops.SlotStats(B, cif, "cuda"), x, prep=dict(gain=gain, noise=noise, ns=ns, stats=ops.SlotStats(B, cif, "cuda")))
    names["new_prep"] = last_kernel()


cases = [("old_conv", old_conv), ("old_pass", old_pass), ("old_pair", old_pair), ("new_plain", new_plain), ("new_prep", new_prep)]
old_conv()
res = {k: [] for k, _ in cases}
for _ in range(rounds):
    for k, f in cases:
        res[k].append(timeit(f))
gb = (gz.numel() + 3 * x.numel()) * 2 / 1e9          # g_z + dot_src + addend in, result out
print(f"B={B} {2 * R}^2 -> {R}^2, {cof} -> {cif} channels, {gb:.3f} GB for the fused form; us per call (SlotStats allocation included), {rounds} interleaved rounds")
for k, _ in cases:
    v = sorted(res[k])
    med = v[len(v) // 2]
    print(f"{k:>10} median {med:8.1f}  min {v[0]:8.1f}  max {v[-1]:8.1f}  {gb / med * 1e3 if k.startswith('new') else 0:5.2f} TB/s  {names.get(k, 'modconv_bwd_prep')}")
