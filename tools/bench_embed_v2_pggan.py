"""Timing of the PGGAN inversion loop (dge_amd.embedding_v2_pggan: PGGAN-1024 + E_PG(16, 9 blocks)) - dev/bench tool.  Random-init
weights, seeded stand-in LPIPS, bf16, mode W.
    python tools/bench_embed_v2_pggan.py [--batches 1,8] [--iters 5] [--rounds 5] [--out profiles/embed_v2_pggan.txt]
Per batch size, in one process, the configurations alternating round by round, medians over --rounds rounds:
  ms/iteration of the eager iteration and of the replayed captured iteration, each with the fused generator backward
  (ops.pixelnorm_act_bwd) and with the composed launches (nearest_up2_bwd -> pixelnorm_nhwc_bwd -> act_bwd);
  the generator backward stage alone (PGGANGenerator._backward on saved activations), fused and composed;
  --layers: every [nearest_up2_bwd ->] pixelnorm_nhwc_bwd -> act_bwd group of that backward on its own shape, fused against composed.
The printed lines (and one JSON line) also go to --out."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd  # noqa: F401
from dge_amd import ops
from dge_amd.embedding_v2_pggan import PGEmbedStep, build_models_pg_v2

ap = argparse.ArgumentParser()
ap.add_argument("--img-size", type=int, default=1024); ap.add_argument("--start-features", type=int, default=16)
ap.add_argument("--batches", default="1,8"); ap.add_argument("--iters", type=int, default=5); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--dtype", default="bf16"); ap.add_argument("--layers", action="store_true"); ap.add_argument("--out", default=None)
a = ap.parse_args()
res, lines = {}, []


def say(s):
    print(s, flush=True)
    lines.append(s)


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


def alternate(runs, n):
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, run in runs.items():
            ms[k].append(timed(run, n))
    return ms


def bench_batch(B):
    img = torch.tanh(torch.randn(B, 3, a.img_size, a.img_size, generator=torch.Generator().manual_seed(7)) * 0.8).cuda()
    z0 = torch.randn(B, 512, generator=torch.Generator().manual_seed(8))
    runs = {}
    for launch in ("eager", "replay"):
        for fused in (True, False):
            G, E, LP = build_models_pg_v2(a.img_size, a.start_features, a.dtype, seed=0)
            st = PGEmbedStep(G, E, LP, mode="W")
            st.fused_backward = fused
            st.begin_image(img, w_init=z0)
            if launch == "replay":
                st.capture(img, warmup=2)
                run = st.replay
            else:
                run = lambda st=st: st.step(img)
                for _ in range(2):
                    run()
            runs[f"{launch}_{'fused' if fused else 'composed'}"] = run
    # the generator backward stage alone, on the saved activations of one forward
    G = build_models_pg_v2(a.img_size, a.start_features, a.dtype, seed=0, lpips=False)[0]
    with torch.no_grad():
        _, _, saved = G._run(z0.cuda(), save=True)
    gimg = torch.randn(B, 3, a.img_size, a.img_size, device="cuda")
    for fused in (True, False):
        def run(fused=fused):
            with torch.no_grad():
                G._backward(saved, gimg, fused)
        for _ in range(2):
            run()
        runs[f"gen_bwd_{'fused' if fused else 'composed'}"] = run
    ms = alternate(runs, a.iters)
    for k, v in ms.items():
        res[f"B{B}_{k}"] = dict(ms=round(median(v), 3), rounds=[round(q, 3) for q in v])
        say(f"embedding_v2_pggan mode W, PGGAN-{a.img_size} + E_PG({a.start_features}), batch {B}, {a.dtype}, {k}: {median(v):.3f} ms")
    if a.layers:
        for L, x_in, y, up in saved["convs"][1:]:          # x_in: the previous conv's output, read by the pixel norm in front of L
            g = torch.randn((B, (2 if up else 1) * x_in.shape[1], (2 if up else 1) * x_in.shape[2], x_in.shape[3]), device="cuda").to(x_in.dtype)

            def composed(g=g, x_in=x_in, up=up):
                gl = ops.nearest_up2_bwd(g)[0] if up else g
                ops.act_bwd(ops.pixelnorm_nhwc_bwd(gl, x_in), x_in, None, pool=False, scale=1.0)
            pair = {"fused": lambda g=g, x_in=x_in, up=up: ops.pixelnorm_act_bwd(g, x_in, up=up), "composed": composed}
            for f in pair.values():
                f()
            t = alternate(pair, 20)
            key = f"B{B}_layer_{x_in.shape[1]}x{x_in.shape[2]}x{x_in.shape[3]}_{'up' if up else 'same'}"
            res[key] = {k: round(median(v) * 1e3, 1) for k, v in t.items()}
            say(f"{key} (us, host-timed over 20 back-to-back launches): fused {median(t['fused']) * 1e3:.1f}, composed {median(t['composed']) * 1e3:.1f}")


for B in [int(v) for v in a.batches.split(",")]:
    bench_batch(B)
say(json.dumps(res))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
