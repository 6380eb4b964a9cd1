"""ms/iteration of the v2 inversion loop (dge_amd.embedding_v2: StyleGAN2 FFHQ-1024 + E_Blur, batch 1) in eager and hipGraph-replay
launch, W+ optimisation and encoder fine-tuning - dev/bench tool.  Random-init weights, seeded stand-in LPIPS.
    python tools/bench_embed_v2.py [--img-size 1024] [--iters 20] [--dtype bf16]
--independent: W mode under hipGraph replay instead - batch 1 on the coupled path against B independent rows per iteration
(--batches 2,4,8), one process, the configurations alternating, medians over --rounds rounds; then the loss stage of one iteration
apart: the per-sample kernels (losses.image_loss_tsa_rows) against the per-row composition (image_loss_tsa on every one-row slice).
    python tools/bench_embed_v2.py --independent [--batches 2,4,8] [--rounds 5]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd  # noqa: F401
from dge_amd.embedding_v2 import LatentEmbedStep, build_models_v2

ap = argparse.ArgumentParser()
ap.add_argument("--img-size", type=int, default=1024); ap.add_argument("--start-features", type=int, default=16)
ap.add_argument("--iters", type=int, default=20); ap.add_argument("--dtype", default="bf16")
ap.add_argument("--independent", action="store_true"); ap.add_argument("--batches", default="2,4,8"); ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
res = {}


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


def bench_independent():
    from dge_amd import losses
    from dge_amd.embedding_v2 import IMG_WEIGHTS
    batches = [int(v) for v in a.batches.split(",")]
    G, E, LP = build_models_v2(2, a.img_size, a.start_features, a.dtype, seed=0)
    with torch.no_grad():
        imgs = G.synthesis(torch.randn(max(batches), G.synthesis.num_layers, 512, device="cuda"))["image"].detach().clamp(-1, 1).contiguous()
    runs = {}
    for name, B, ind in [("B1_coupled", 1, False)] + [(f"B{B}_independent", B, True) for B in batches]:
        st = LatentEmbedStep(G, E, LP, mode="W", generator="sg2", independent=ind)
        st.begin_image(imgs[:B].contiguous())
        st.capture(imgs[:B].contiguous(), warmup=1)
        for _ in range(3):
            st.replay()
        runs[name] = (st, B)
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name, (st, B) in runs.items():
            ms[name].append(timed(st.replay, a.iters))
    for name, (st, B) in runs.items():
        m = median(ms[name])
        res[name] = dict(ms_per_iteration=round(m, 3), ms_per_image_iteration=round(m / B, 3), rounds=[round(v, 3) for v in ms[name]])
        print(f"embedding_v2 W replay, StyleGAN2-{a.img_size} + E_Blur, {a.dtype}, {name}: {m:.2f} ms/iteration, {m / B:.2f} ms/image-iteration", flush=True)
    runs.clear()
    # the loss stage of one iteration (value + analytic gradient of the three windows), eager launches
    for B in batches:
        x = imgs[:B].contiguous()
        y = (x * 0.9 + 0.05 * torch.randn_like(x)).requires_grad_(True)
        rows = lambda: losses.image_loss_tsa_rows(x, y, LP, IMG_WEIGHTS)
        xs, ys = [x[r:r + 1].contiguous() for r in range(B)], [y.detach()[r:r + 1].contiguous().requires_grad_(True) for r in range(B)]
        comp = lambda: [losses.image_loss_tsa(xs[r], ys[r], LP, IMG_WEIGHTS) for r in range(B)]
        for f in (rows, comp, rows, comp):
            f()
        t = {"rows": [], "composition": []}
        for _ in range(a.rounds):
            t["rows"].append(timed(rows, a.iters))
            t["composition"].append(timed(comp, a.iters))
        res[f"loss_stage_B{B}"] = {k: dict(ms=round(median(v), 3), rounds=[round(q, 3) for q in v]) for k, v in t.items()}
        print(f"loss stage, B = {B}: per-sample kernels {median(t['rows']):.2f} ms, per-row composition {median(t['composition']):.2f} ms", flush=True)
    print(json.dumps(res))


if a.independent:
    bench_independent()
    sys.exit(0)
for mode in ("W", "E"):
    G, E, LP = build_models_v2(2, a.img_size, a.start_features, a.dtype, seed=0)
    with torch.no_grad():
        imgs1 = G.synthesis(torch.randn(1, G.synthesis.num_layers, 512, device="cuda"))["image"].detach().clamp(-1, 1).contiguous()
    for launch in ("eager", "graph"):
        st = LatentEmbedStep(G, E, LP, mode=mode, generator="sg2")
        st.begin_image(imgs1)
        if launch == "graph":
            st.capture(imgs1, warmup=1)
            run = st.replay
        else:
            run = lambda: st.step(imgs1)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(a.iters):
            run()
        torch.cuda.synchronize()
        dt = (time.time() - t0) / a.iters
        res[f"{mode}_{launch}_ms"] = round(dt * 1e3, 2)
        print(f"embedding_v2 loop, StyleGAN2-{a.img_size} + E_Blur, batch 1, {a.dtype}, mode {mode}, {launch}: {dt * 1e3:.2f} ms/iteration",
              flush=True)
        del st
print(json.dumps(res))
