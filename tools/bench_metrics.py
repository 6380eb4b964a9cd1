"""Time of the per-image evaluation metrics (infer.image_metrics_rows: PSNR / SSIM / MSE / cosine of every pair on 8-bit images) at
[1,1024,1024,3] and [8,1024,1024,3] against the way to per-image numbers without it - infer.image_metrics on every one-row slice
(dge_loss_reduce + dge_ssim_box7 per image, float [-1,1] inputs) - dev/bench tool.
    python tools/bench_metrics.py [--size 1024] [--batches 1,8] [--iters 200] [--rounds 5] [--out FILE]
One process, the configurations alternating round by round, medians over --rounds rounds; host clock around --iters back-to-back
calls that end in a device synchronise.  Configurations:
  metrics_u8    one dge_image_metrics_u8 launch (+ its finaliser) on uint8 images already on the device (decoded files);
  rows_bf16     the same after two dge_quantize_u8 launches from bf16 [B,3,H,W] images (generator output);
  composition   image_metrics(a[r:r+1], b[r:r+1]) for every row r on the same bf16 images.
Bytes the metrics launch has to read: 2 * B * H * W * 3 (50 MB at B = 8); the GB/s printed is that over the launch time."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd  # noqa: F401
from dge_amd import infer

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024); ap.add_argument("--batches", default="1,8")
ap.add_argument("--iters", type=int, default=200); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_metrics: needs the GPU (a CPU run measures nothing)")


def timed(run, n):
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(n):
        run()
    torch.cuda.synchronize()
    return (time.time() - t0) / n * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


res = {}
for B in [int(v) for v in a.batches.split(",")]:
    gen = torch.Generator(device="cuda").manual_seed(B)
    x = torch.rand(B, 3, a.size, a.size, device="cuda", generator=gen) * 2 - 1
    y = (x * 0.9 + 0.1 * torch.randn(x.shape, device="cuda", generator=gen)).clamp(-1, 1)
    x, y = x.to(torch.bfloat16), y.to(torch.bfloat16)
    qx, qy = infer.quantize_u8(x), infer.quantize_u8(y)
    xs, ys = [x[r:r + 1] for r in range(B)], [y[r:r + 1] for r in range(B)]
    cfg = {"metrics_u8": lambda: infer.image_metrics_rows(qx, qy),
           "rows_bf16": lambda: infer.image_metrics_rows(x, y),
           "composition": lambda: [infer.image_metrics(xs[r], ys[r]) for r in range(B)]}
    for f in cfg.values():
        for _ in range(3):
            f()
    # the two ways measure different images (8-bit against float): what they report for row 0, for the record
    m, c = infer.image_metrics_rows(x, y), infer.image_metrics(xs[0], ys[0])
    diff = {k: abs(float(m[k][0]) - float(c[k])) for k in ("psnr", "ssim", "mse", "cosine")}
    t = {k: [] for k in cfg}
    for _ in range(a.rounds):
        for k, f in cfg.items():
            t[k].append(timed(f, a.iters))
    med = {k: median(v) for k, v in t.items()}
    mb = 2 * B * a.size * a.size * 3 / 1e6
    res[f"B{B}"] = dict({k: dict(ms=round(med[k], 4), rounds=[round(q, 4) for q in v]) for k, v in t.items()},
                        input_MB=round(mb, 1), metrics_u8_GBps=round(mb / med["metrics_u8"], 1),
                        composition_over_rows_bf16=round(med["composition"] / med["rows_bf16"], 2),
                        composition_over_metrics_u8=round(med["composition"] / med["metrics_u8"], 2), row0_abs_diff_8bit_vs_float=diff)
    print(f"[{B},{a.size},{a.size},3] (ms, host-timed over {a.iters} back-to-back calls, medians of {a.rounds} rounds): "
          + ", ".join(f"{k} {v:.3f}" for k, v in med.items())
          + f"; metrics_u8 reads {mb:.1f} MB = {mb / med['metrics_u8']:.1f} GB/s; composition / rows_bf16 = {med['composition'] / med['rows_bf16']:.2f}x",
          flush=True)
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
