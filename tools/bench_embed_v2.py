"""ms/iteration of the v2 inversion loop (dge_amd.embedding_v2: StyleGAN2 FFHQ-1024 + E_Blur, batch 1) in eager and hipGraph-replay
launch, W+ optimisation and encoder fine-tuning - dev/bench tool.  Random-init weights, seeded stand-in LPIPS.
    python tools/bench_embed_v2.py [--img-size 1024] [--iters 20] [--dtype bf16]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd  # noqa: F401
from dge_amd.embedding_v2 import LatentEmbedStep, build_models_v2

ap = argparse.ArgumentParser()
ap.add_argument("--img-size", type=int, default=1024); ap.add_argument("--start-features", type=int, default=16)
ap.add_argument("--iters", type=int, default=20); ap.add_argument("--dtype", default="bf16")
a = ap.parse_args()
res = {}
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
