"""Timing of the region directions (dge_amd.region_directions; README, "Region directions") - dev/bench tool, one process.
  * dge_gram_cols at K = 512 with the mask weight (both Grams from one read) at N = 3 * 256^2 and N = 3 * 1024^2 columns: device
    events around --iters calls; beside it, for context only, torch's (X * w) @ X^T on the same operand (ONE of the two Grams, and a
    second pass over X to scale it), in the same process, the two alternating round by round;
  * the whole fit (region_directions: 512 axes, one code, one mask) on StyleGAN2-<img-size> with random-init weights at jac_res 256
    and jac_res = img-size: host clock around one call that ends in a device synchronise.  A fit is long: after one warm-up call
    the rounds are min(--rounds, --fit-budget seconds / the warm-up's time), at least one, and the line says how many ran.
Medians over the rounds with the round spread (max - min).
    python tools/bench_region_directions.py [--img-size 1024] [--dtype f32] [--iters 3] [--rounds 5] [--fit-budget 120] [--skip-fit]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd  # noqa: F401
from dge_amd import ops
from dge_amd.region_directions import region_directions

ap = argparse.ArgumentParser()
ap.add_argument("--img-size", type=int, default=1024); ap.add_argument("--dtype", default="f32")
ap.add_argument("--fmaps-base", type=int, default=None); ap.add_argument("--fmaps-max", type=int, default=None)
ap.add_argument("--iters", type=int, default=3); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--axes", type=int, default=512); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--fit-budget", type=float, default=120.0); ap.add_argument("--skip-fit", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_region_directions needs the GPU"
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


def report(name, v, note=""):
    m, spread = median(v), max(v) - min(v)
    res[name] = dict(ms=round(m, 4), spread=round(spread, 4), rounds=[round(q, 4) for q in v])
    print(f"{name}: {m:.3f} ms (spread {spread:.3f}, {len(v)} rounds){note}", flush=True)


K = a.axes
for r in (256, 1024):
    N, P = 3 * r * r, r * r
    g = torch.Generator(device="cuda").manual_seed(r)
    X = torch.empty((K, N), dtype=torch.float32, device="cuda")
    for k0 in range(0, K, 64):                                        # filled in pieces: randn's temporaries stay small
        X[k0:k0 + 64].normal_(generator=g)
    w = torch.rand(P, generator=g, device="cuda")
    wfull = w.repeat(3)
    ours, ref = (lambda: ops.gram_cols(X, wgt=w)), (lambda: (X * wfull) @ X.t())
    Ma, _ = ours()
    Mt = ref()
    rel = float((Ma - Mt).abs().max() / Mt.abs().max())
    torch.cuda.synchronize()
    t_ours, t_ref = [], []
    for _ in range(a.rounds):
        t_ours.append(device_ms(ours, a.iters))
        t_ref.append(device_ms(ref, a.iters))
    flop = 2.0 * K * K * N
    bytes_x = 4.0 * K * N
    m = median(t_ours)
    report(f"gram_cols_{K}x3x{r}x{r}", t_ours, f", both Grams: {2 * flop / m * 1e-9:.1f} TFLOP/s as two full products (the kernel computes the upper "
           f"triangle: {2 * flop * (K / 64 + 1) / (2 * K / 64) / m * 1e-9:.1f}), operand {bytes_x * 1e-9:.2f} GB, chunk {ops.gram_cols_chunk(N)} columns")
    report(f"torch_xw_xt_{K}x3x{r}x{r}", t_ref, f", ONE Gram: {flop / median(t_ref) * 1e-9:.1f} TFLOP/s; max |ours - torch| / max = {rel:.2e}")
    res[f"gram_cols_{K}x3x{r}x{r}_vs_torch_rel"] = rel
    del X, w, wfull, Ma, Mt, ours, ref
    torch.cuda.empty_cache()

if not a.skip_fit:
    kw = {k: v for k, v in (("fmaps_base", a.fmaps_base), ("fmaps_max", a.fmaps_max)) if v is not None}
    torch.manual_seed(0)
    G = dge_amd.StyleGAN2Generator(a.img_size, compute_dtype=a.dtype, **kw).cuda()
    G.eval()
    S = a.img_size
    wp = torch.randn(1, G.synthesis.num_layers, 512, generator=torch.Generator().manual_seed(1)).cuda()
    mask = torch.zeros(1, 1, S, S, device="cuda")
    mask[:, :, S // 4:S // 2, S // 4:3 * S // 4] = 1.0
    basis = None if K == 512 else torch.eye(512, device="cuda")[:K].contiguous()
    for r in sorted({min(256, S), S}):
        fit = lambda: region_directions(G, [wp], [mask], basis=basis, jac_res=r, batch=a.batch)
        warm = host_ms(fit)
        rounds = max(1, min(a.rounds, int(a.fit_budget * 1e3 / warm)))
        print(f"fit_jac_res_{r}: warm-up call {warm:.1f} ms, timing {rounds} rounds", flush=True)
        v = []
        for _ in range(rounds):
            v.append(host_ms(fit))
        report(f"fit_jac_res_{r}", v, f", StyleGAN2-{S} random-init {a.dtype}, {K} axes, {2 * K} images in calls of {a.batch}")
print(json.dumps(res))
