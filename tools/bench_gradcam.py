"""Attention-map path timing: Grad-CAM++ masks + guided back-propagation + mask2cam of one image
batch on the full VGG16 widths (stand-in weights), and the whole E_mis_align_cropping_s1 iteration - dev/bench tool.
    python tools/bench_gradcam.py [--img-size 256] [--batch 5] [--iters 10] [--step]
    python tools/bench_gradcam.py --compare [--img-size 1024 --batch 8 --start-features 16 --iters 5]
--compare: the pair pass (both image batches through VGG16 once) against two fused passes, for the attention alone and inside the
s1 and case 2 iterations of dge_amd.mis_align."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd
from dge_amd import grad_cam as G
ap = argparse.ArgumentParser()
ap.add_argument("--img-size", type=int, default=256); ap.add_argument("--batch", type=int, default=5)
ap.add_argument("--iters", type=int, default=10); ap.add_argument("--dtype", default="bf16")
ap.add_argument("--step", action="store_true", help="time the whole mis-align iteration (StyleGAN2 + E.BE + LPIPS + attention maps)")
ap.add_argument("--start-features", type=int, default=64)
ap.add_argument("--compare", action="store_true", help="pair pass against two fused passes - the attention alone and the whole s1 / case 2 "
                "iteration - in ONE process, the configurations alternating round by round: medians of --rounds rounds and their spread, "
                "one JSON line per measurement")
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
net = G.VGG16(compute_dtype=a.dtype).cuda()


def compare():
    import json, statistics
    from dge_amd.e_align import build_models
    from dge_amd.mis_align import MisAlignStep
    gcpp = G.GradCamPlusPlus(net, net.final_layer)
    G.GuidedBackPropagation(net)
    B, R = a.batch, a.img_size
    imgs1 = torch.randn(B, 3, R, R, device="cuda").clamp(-1, 1)
    imgs2 = torch.randn(B, 3, R, R, device="cuda").clamp(-1, 1)

    def att_fused():
        for imgs in (imgs1, imgs2):
            mask, _ = gcpp.with_input_gradient(imgs)
            G.mask2cam(mask, imgs)

    def att_pair():
        gcpp.with_input_gradient_pair(imgs1, imgs2)
        G.mask2cam(gcpp.pair_mask, torch.cat((imgs1, imgs2)), groups=2)
    Gen, E, LP = build_models(R, a.start_features, a.dtype)
    steps = {case: MisAlignStep(Gen, E, LP, net, batch_size=B, case=case) for case in ("s1", "case2")}      # (one encoder, two optimizers)
    it = [0]

    def iteration(case, attention):
        def run():
            steps[case].attention = attention
            steps[case].step(it[0]); it[0] += 1
        return run
    configs = {"attention/fused": att_fused, "attention/pair": att_pair}
    for case in steps:
        for attention in ("fused", "pair"):
            configs[f"{case}/{attention}"] = iteration(case, attention)
    times = {k: [] for k in configs}
    for rnd in range(a.rounds + 1):                      # round 0 warms every configuration up and is dropped
        for name, run in configs.items():
            run()
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(a.iters):
                run()
            torch.cuda.synchronize()
            if rnd:
                times[name].append((time.time() - t0) / a.iters * 1e3)
    for name, ts in times.items():
        print(json.dumps(dict(config=name, batch=B, img_size=R, dtype=a.dtype, iters=a.iters, median_ms=round(statistics.median(ts), 3),
                              min_ms=round(min(ts), 3), max_ms=round(max(ts), 3), rounds_ms=[round(t, 3) for t in ts])), flush=True)


if a.compare:
    compare()
    sys.exit(0)
if a.step:
    from dge_amd.e_align import build_models
    from dge_amd.mis_align import MisAlignStep
    Gen, E, LP = build_models(a.img_size, a.start_features, a.dtype)
    st = MisAlignStep(Gen, E, LP, net, batch_size=a.batch)
    it = [0]
    def run():
        st.step(it[0]); it[0] += 1
    what = f"E_mis_align_cropping_s1 iteration, StyleGAN2-{a.img_size} + E.BE(startf={a.start_features}) + VGG16 attention maps"
else:
    gcpp = G.GradCamPlusPlus(net, net.final_layer)
    gbp = G.GuidedBackPropagation(net)
    imgs = torch.randn(a.batch, 3, a.img_size, a.img_size, device="cuda").clamp(-1, 1)
    def run():
        mask, _ = gcpp.with_input_gradient(imgs)
        G.mask2cam(mask, imgs)
    what = f"Grad-CAM++ mask + guided back-propagation + mask2cam, VGG16 @ {a.img_size}^2"
for i in range(3):
    run()
torch.cuda.synchronize()
t0 = time.time()
for i in range(a.iters):
    run()
torch.cuda.synchronize()
dt = (time.time() - t0) / a.iters
print(f"{what}, batch {a.batch}, {a.dtype}: {dt*1e3:.2f} ms/iteration, {a.batch/dt:.1f} img/s")
