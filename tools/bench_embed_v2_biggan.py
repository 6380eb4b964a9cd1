"""Timing of the BigGAN-deep inversion loop (dge_amd.embedding_v2_biggan: BigGAN-deep-256 + E_BIG) - dev/bench tool.  Random-init
weights, seeded stand-in LPIPS and vgg16.
    python tools/bench_embed_v2_biggan.py [--batch 1] [--iters 10] [--rounds 5] [--dtype bf16] [--attention false]
ms/iteration of the eager iteration (there is no captured form) in mode W and mode E, with the last backward stage of E(imgs2) as
one launch and as the composed launches (autograd_encbig.FUSE_IMG_GRAD) - four configurations in one process, alternating round by
round, medians over --rounds rounds.
--last-stage: the last stage of the E_BIG backward alone when the image carries a gradient, at [B,256,256,64] for B in --batches:
the one launch (ops.affine_bwd_fromrgb_img) against the launches it replaces (in_bwd with (a, 0, 0) -> fromrgb_dgrad
[-> fromrgb_bwd]), frozen and trained encoder, alternating, medians over --rounds rounds.
    python tools/bench_embed_v2_biggan.py --last-stage --batches 1,8
--independent: mode W, batch 1 on the coupled BigEmbedStep against the independent rows (BigEmbedRowsStep, labels 30, 207, 5, ...) at
every B of --batches - one process, the configurations alternating round by round, medians over --rounds rounds, with the
round-to-round spread (max - min over the median) of every configuration.
    python tools/bench_embed_v2_biggan.py --independent --batches 1,2,4,8"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd  # noqa: F401
from dge_amd import autograd_encbig, ops
from dge_amd.embedding_v2 import strict_bool
from dge_amd.embedding_v2_biggan import BigEmbedRowsStep, BigEmbedStep, build_models_big_v2

ap = argparse.ArgumentParser()
ap.add_argument("--img-size", type=int, default=256); ap.add_argument("--start-features", type=int, default=64)
ap.add_argument("--batch", type=int, default=1); ap.add_argument("--iters", type=int, default=10); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--dtype", default="bf16"); ap.add_argument("--attention", type=strict_bool, default=True)
ap.add_argument("--last-stage", action="store_true"); ap.add_argument("--batches", default="1,8")
ap.add_argument("--independent", action="store_true")
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


def bench_last_stage():
    """Synthetic operands of block 0's last stage (conv_1's data gradient g_u1, the FromRGB output x0, the pooled skip gradient)."""
    R_, C = a.img_size, a.start_features
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    for B in [int(v) for v in a.batches.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(B)
        rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
        gy, x0, extra = rn(B, R_, R_, C).to(dt), rn(B, R_, R_, C).to(dt), rn(B, R_ // 2, R_ // 2, C).to(dt)
        av, w, img = rn(B, C).abs() + 0.5, rn(C, 3, 1, 1), rn(B, 3, R_, R_)
        kw = dict(extra=extra, extra_pool=True, extra_scale=0.25)

        def composed(params):
            gx0 = ops.in_bwd(gy, x0, autograd_encbig._affine_coef(av), **kw)
            ops.fromrgb_dgrad(gx0, x0, w)
            if params:
                ops.fromrgb_bwd(gx0, x0, img)
        cfg = {"frozen_fused": lambda: ops.affine_bwd_fromrgb_img(gy, x0, av, w, None, **kw), "frozen_composed": lambda: composed(False),
               "trained_fused": lambda: ops.affine_bwd_fromrgb_img(gy, x0, av, w, img, **kw), "trained_composed": lambda: composed(True)}
        for f in cfg.values():
            for _ in range(3):
                f()
        t = {k: [] for k in cfg}
        for _ in range(a.rounds):
            for k, f in cfg.items():
                t[k].append(timed(f, a.iters) * 1e3)
        res[f"last_stage_B{B}"] = {k: dict(us=round(median(v), 1), rounds=[round(q, 1) for q in v]) for k, v in t.items()}
        print(f"last backward stage [{B},{R_},{R_},{C}] {a.dtype} (us, host-timed over {a.iters} back-to-back launches): "
              + ", ".join(f"{k} {median(v):.1f}" for k, v in t.items()), flush=True)
    print(json.dumps(res))


def bench_loop():
    B = a.batch
    runs = {}
    for mode in ("W", "E"):
        G, E, LP, vgg = build_models_big_v2(None, a.img_size, a.start_features, a.dtype, seed=0, attention=a.attention)
        st = BigEmbedStep(G, E, LP, mode=mode, vgg16=vgg, attention=a.attention, iterations=1501)
        st._setup((st.label,) * B, torch.device("cuda", torch.cuda.current_device()))
        with torch.no_grad():
            imgs1 = G(st.cond_vector[:, :G.config.z_dim].contiguous(), st.conditions, st.truncation)[0].detach().clamp(-1, 1).contiguous()
        st.begin_image(imgs1)
        for fused in (True, False):
            def run(st=st, imgs1=imgs1, fused=fused):
                autograd_encbig.FUSE_IMG_GRAD = fused
                st.step(imgs1)
            for _ in range(2):
                run()
            runs[f"{mode}_{'fused' if fused else 'composed'}"] = run
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, run in runs.items():
            ms[k].append(timed(run, a.iters))
    autograd_encbig.FUSE_IMG_GRAD = True
    for k, v in ms.items():
        res[k] = dict(ms_per_iteration=round(median(v), 3), rounds=[round(q, 3) for q in v])
        print(f"embedding_v2_biggan eager, BigGAN-deep-{a.img_size} + E_BIG, batch {B}, {a.dtype}, attention {a.attention}, {k}: "
              f"{median(v):.2f} ms/iteration", flush=True)
    print(json.dumps(res))


def bench_independent():
    G, E, LP, vgg = build_models_big_v2(None, a.img_size, a.start_features, a.dtype, seed=0, attention=a.attention)
    dev = torch.device("cuda", torch.cuda.current_device())
    labels = [30, 207, 5, 1, 9, 100, 417, 980]
    runs = {}

    def add(name, st, B, **kw):
        st._setup(tuple(labels[b % 8] for b in range(B)) if kw else (st.label,) * B, dev)
        with torch.no_grad():
            imgs1 = G(st.cond_vector[:, :G.config.z_dim].contiguous(), st.conditions, st.truncation)[0].detach().clamp(-1, 1).contiguous()
        runs[name] = (st, imgs1, B, kw)

    add("coupled_B1", BigEmbedStep(G, E, LP, mode="W", vgg16=vgg, attention=a.attention, iterations=1501), 1)
    for B in [int(v) for v in a.batches.split(",")]:
        add(f"rows_B{B}", BigEmbedRowsStep(G, E, LP, vgg16=vgg, attention=a.attention, iterations=1501), B, labels=[labels[b % 8] for b in range(B)])
    for st, imgs1, B, kw in runs.values():          # (the steps share G and E: mode W leaves both unchanged but for the u / v buffers)
        st.begin_image(imgs1, **kw)
        for _ in range(2):
            st.step(imgs1)
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, (st, imgs1, B, kw) in runs.items():
            ms[k].append(timed(lambda: st.step(imgs1), a.iters))
    for k, v in ms.items():
        B = runs[k][2]
        m = median(v)
        res[k] = dict(ms_per_iteration=round(m, 3), ms_per_image_iteration=round(m / B, 3), spread=round((max(v) - min(v)) / m, 4),
                      rounds=[round(q, 3) for q in v])
        print(f"embedding_v2_biggan eager mode W, BigGAN-deep-{a.img_size} + E_BIG, {a.dtype}, attention {a.attention}, {k}: "
              f"{m:.2f} ms/iteration, {m / B:.2f} ms/image-iteration, round-to-round spread {100 * (max(v) - min(v)) / m:.1f} %", flush=True)
    print(json.dumps(res))


bench_last_stage() if a.last_stage else (bench_independent() if a.independent else bench_loop())
