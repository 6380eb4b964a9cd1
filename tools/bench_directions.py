"""Timing of the semantic directions (dge_amd.directions; README, "Semantic directions") - dev/bench tool, one process.
  * dge_gram at the two operand sizes of the workload, 10 000 x 512 (the W-space PCA; with the mean) and 9088 x 512 (SeFa over all
    blocks of StyleGAN2-1024; with the row norms): device events around --iters calls;
  * dge_eigh_sym at D = 512 on the Gram matrix of 2048 unit rows: device events around --iters calls (each call reads the host once
    per sweep), the sweeps it took, and beside it torch.linalg.eigh on the CPU of the same machine for the same matrix (host clock);
  * the two fits, sefa_directions and pca_directions, on StyleGAN2-<img-size> with random-init weights: host clock around one call
    that ends in a device synchronise.
Medians over --rounds rounds with the round spread (max - min).
    python tools/bench_directions.py [--img-size 1024] [--dtype bf16] [--iters 5] [--rounds 5] [--samples 10000]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd  # noqa: F401
from dge_amd import ops
from dge_amd.directions import pca_directions, sefa_directions

ap = argparse.ArgumentParser()
ap.add_argument("--img-size", type=int, default=1024); ap.add_argument("--dtype", default="bf16")
ap.add_argument("--fmaps-base", type=int, default=None); ap.add_argument("--fmaps-max", type=int, default=None)
ap.add_argument("--iters", type=int, default=5); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--samples", type=int, default=10000)
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_directions needs the GPU"
res = {}


def device_ms(run, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def host_ms(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def report(ms, note={}):
    for name, v in ms.items():
        m, spread = median(v), max(v) - min(v)
        res[name] = dict(ms=round(m, 4), spread=round(spread, 4), rounds=[round(q, 4) for q in v])
        print(f"{name}: {m:.3f} ms (spread {spread:.3f}){note.get(name, '')}", flush=True)


g = torch.Generator().manual_seed(0)
x_pca, x_sefa = torch.randn(10000, 512, generator=g).cuda(), torch.randn(9088, 512, generator=g).cuda()
mean = x_pca.mean(0).contiguous()
rows = torch.randn(2048, 512, generator=g)
rows = (rows / rows.norm(dim=1, keepdim=True)).cuda()
M = ops.gram(rows)
runs = {"gram_10000x512_mean": lambda: ops.gram(x_pca, mean=mean, scale=1e-4),
        "gram_9088x512_row_norm": lambda: ops.gram(x_sefa, row_norm=True),
        "eigh_sym_512": lambda: ops.eigh_sym(M)}
for run in runs.values():
    run()
ms = {k: [] for k in runs}
for _ in range(a.rounds):
    for name, run in runs.items():
        ms[name].append(device_ms(run, a.iters))
sweeps, off = ops.eigh_sym(M)[2]
res["eigh_sym_512_sweeps"], res["eigh_sym_512_off"], res["eigh_sym_512_launches_per_sweep"] = sweeps, off, 511 + 2
flops = {"gram_10000x512_mean": 2 * 10000 * 512 * 512, "gram_9088x512_row_norm": 2 * 9088 * 512 * 512}
report(ms, {k: f", {v / 1e9:.2f} GFLOP as a full product" for k, v in flops.items()} |
       {"eigh_sym_512": f", {sweeps} sweeps of 511 + 2 launches, off(A) {off:.2e}"})

Mh = M.cpu()
cpu = []
for _ in range(a.rounds):
    t0 = time.perf_counter()
    torch.linalg.eigh(Mh)
    cpu.append((time.perf_counter() - t0) * 1e3)
report({"torch_linalg_eigh_cpu_512": cpu}, {"torch_linalg_eigh_cpu_512": f" on {torch.get_num_threads()} threads, f32"})

torch.manual_seed(0)
kw = {k: v for k, v in (("fmaps_base", a.fmaps_base), ("fmaps_max", a.fmaps_max)) if v is not None}
G = dge_amd.StyleGAN2Generator(a.img_size, compute_dtype=a.dtype, **kw).cuda()
G.eval()
fits = {"fit_sefa": lambda: sefa_directions(G), "fit_pca": lambda: pca_directions(G, samples=a.samples)}
for run in fits.values():
    run()
ms = {k: [] for k in fits}
for _ in range(a.rounds):
    for name, run in fits.items():
        ms[name].append(host_ms(run))
report(ms, {"fit_sefa": f", StyleGAN2-{a.img_size} random-init, all rows", "fit_pca": f", StyleGAN2-{a.img_size} random-init, {a.samples} samples"})
print(json.dumps(res))
