"""ms/iteration of the v2 inversion loop (dge_amd.embedding_v2: StyleGAN2 FFHQ-1024 + E_Blur, batch 1) in eager and hipGraph-replay
launch, W+ optimisation and encoder fine-tuning - dev/bench tool.  Random-init weights, seeded stand-in LPIPS.
    python tools/bench_embed_v2.py [--img-size 1024] [--iters 20] [--dtype bf16]
--independent: W mode under hipGraph replay instead - batch 1 on the coupled path against B independent rows per iteration
(--batches 2,4,8), one process, the configurations alternating, medians over --rounds rounds; then the loss stage of one iteration
apart: the per-sample kernels (losses.image_loss_tsa_rows) against the per-row composition (image_loss_tsa on every one-row slice).
    python tools/bench_embed_v2.py --independent [--batches 2,4,8] [--rounds 5]
--encoder be: E.BE (the encoder E_align trains) in E_Blur's place, in every mode above.
--compare-encoders: W mode under hipGraph replay, E.BE against E_Blur at batch 1 (coupled) and --batches independent rows, one
process, the configurations alternating, medians over --rounds rounds.
--last-stage: the last stage of E.BE's backward alone when the image carries a gradient, at [B,1024,1024,16] for B in --batches:
the one launch (ops.in_bwd_fromrgb_img) against the passes it replaces (in_bwd -> fromrgb_dgrad [-> fromrgb_bwd]), frozen and
trained encoder, alternating, medians over --rounds rounds.
--space z: the Z-space loop (mode "Z") under hipGraph replay at batch 1 (coupled) and --batches independent rows, with each
route of the mapping adjoint (dge_mapping_bwd / dge_mapping_bwd_wide), beside mode W on the same box, one process, the
configurations alternating, medians over --rounds rounds with the round spread.
--optimize_noise: mode W under hipGraph replay with the noise maps optimised beside the W+ code against the same step without
them, at batch 1 (coupled) and the other --batches as independent rows, one process, flag on and off alternating round by round,
medians over --rounds rounds with the round spread; then the noise-gradient passes of one synthesis backward alone (device time
of the per-layer dge_s2_noise_grad launches on operands of the layers' shapes) and the regulariser and renormalisation launches.
    python tools/bench_embed_v2.py --optimize_noise --batches 1,8
    python tools/bench_embed_v2.py --space z --batches 8
    python tools/bench_embed_v2.py --compare-encoders --batches 8
    python tools/bench_embed_v2.py --last-stage --batches 1,8"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd  # noqa: F401
from dge_amd.embedding_v2 import LatentEmbedStep, build_models_v2

ap = argparse.ArgumentParser()
ap.add_argument("--img-size", type=int, default=1024); ap.add_argument("--start-features", type=int, default=16)
ap.add_argument("--iters", type=int, default=20); ap.add_argument("--dtype", default="bf16")
ap.add_argument("--encoder", choices=("blur", "be"), default="blur"); ap.add_argument("--compare-encoders", action="store_true")
ap.add_argument("--last-stage", action="store_true")
ap.add_argument("--space", choices=("w", "z"), default="w")
ap.add_argument("--optimize_noise", action="store_true")
ap.add_argument("--independent", action="store_true"); ap.add_argument("--batches", default="2,4,8"); ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
res = {}
ENC_NAME = {"blur": "E_Blur", "be": "E.BE"}


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
    G, E, LP = build_models_v2(2, a.img_size, a.start_features, a.dtype, seed=0, encoder=a.encoder)
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
        print(f"embedding_v2 W replay, StyleGAN2-{a.img_size} + {ENC_NAME[a.encoder]}, {a.dtype}, {name}: {m:.2f} ms/iteration, {m / B:.2f} ms/image-iteration", flush=True)
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


def bench_space_z():
    batches = [int(v) for v in a.batches.split(",")]
    G, E, LP = build_models_v2(2, a.img_size, a.start_features, a.dtype, seed=0, encoder=a.encoder)
    with torch.no_grad():
        imgs = G.synthesis(torch.randn(max(batches + [1]), G.synthesis.num_layers, 512, device="cuda"))["image"].detach().clamp(-1, 1).contiguous()
    runs = {}
    for shape, B, ind in [("B1_coupled", 1, False)] + [(f"B{B}_independent", B, True) for B in batches]:
        for name, kw in (("W", dict(mode="W")), ("Z_one_launch", dict(mode="Z", mapping_bwd="one")), ("Z_wide", dict(mode="Z", mapping_bwd="wide"))):
            st = LatentEmbedStep(G, E, LP, generator="sg2", independent=ind, **kw)
            st.begin_image(imgs[:B].contiguous())
            st.capture(imgs[:B].contiguous(), warmup=1)
            for _ in range(3):
                st.replay()
            runs[f"{shape}_{name}"] = (st, B)
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name, (st, B) in runs.items():
            ms[name].append(timed(st.replay, a.iters))
    for name, (st, B) in runs.items():
        m = median(ms[name])
        res[name] = dict(ms_per_iteration=round(m, 3), spread=round(max(ms[name]) - min(ms[name]), 3), rounds=[round(v, 3) for v in ms[name]])
        print(f"embedding_v2 replay, StyleGAN2-{a.img_size} + {ENC_NAME[a.encoder]}, {a.dtype}, {name}: {m:.3f} ms/iteration "
              f"(spread {max(ms[name]) - min(ms[name]):.3f}), {m / B:.3f} ms/image-iteration", flush=True)
    print(json.dumps(res))


def bench_noise():
    from dge_amd import ops
    batches = [int(v) for v in a.batches.split(",")]
    G, E, LP = build_models_v2(2, a.img_size, a.start_features, a.dtype, seed=0, encoder=a.encoder)
    with torch.no_grad():
        imgs = G.synthesis(torch.randn(max(batches), G.synthesis.num_layers, 512, device="cuda"))["image"].detach().clamp(-1, 1).contiguous()
    runs = {}
    for B in batches:
        for flag in (False, True):
            st = LatentEmbedStep(G, E, LP, mode="W", generator="sg2", independent=B > 1, optimize_noise=flag)
            st.begin_image(imgs[:B].contiguous())
            st.capture(imgs[:B].contiguous(), warmup=1)
            for _ in range(3):
                st.replay()
            runs[f"B{B}_{'independent' if B > 1 else 'coupled'}_{'noise' if flag else 'plain'}"] = (st, B)
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name, (st, B) in runs.items():
            ms[name].append(timed(st.replay, a.iters))
    for name, (st, B) in runs.items():
        m = median(ms[name])
        res[name] = dict(ms_per_iteration=round(m, 3), spread=round(max(ms[name]) - min(ms[name]), 3), rounds=[round(v, 3) for v in ms[name]])
        print(f"embedding_v2 W replay, StyleGAN2-{a.img_size} + {ENC_NAME[a.encoder]}, {a.dtype}, {name}: {m:.3f} ms/iteration "
              f"(spread {max(ms[name]) - min(ms[name]):.3f}), {m / B:.3f} ms/image-iteration", flush=True)
    # the passes alone, device time between two events around `iters` repetitions
    S = G.synthesis
    layers = [getattr(S, f"layer{i}") for i in range(S.num_layers - 1)]
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32

    def device_ms(f):
        for _ in range(3):
            f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters
    for B in batches:
        Bn = B if B > 1 else 1
        gz = [torch.randn(B, L.res, L.res, L.out_c, device="cuda").to(dt) for L in layers]
        outs = [torch.empty(Bn, L.res * L.res, device="cuda") for L in layers]
        ns = [L.noise_strength.detach().reshape(1) for L in layers]
        tab = ops.NoiseTable([L.res for L in layers], Bn, "cuda")
        flat, grad = torch.randn(tab.numel, device="cuda"), torch.empty(tab.numel, device="cuda")
        nbytes = sum(g.numel() * g.element_size() for g in gz)
        t = dict(noise_grad_form_A=[], noise_grad_form_B=[], noise_reg=[], noise_normalize=[])
        for _ in range(a.rounds):
            t["noise_grad_form_A"].append(device_ms(lambda: [ops.s2_noise_grad(g, None, L.gain, n, o) for g, L, n, o in zip(gz, layers, ns, outs)]))
            t["noise_grad_form_B"].append(device_ms(lambda: [ops.s2_noise_grad(g, g, L.gain, n, o) for g, L, n, o in zip(gz, layers, ns, outs)]))
            t["noise_reg"].append(device_ms(lambda: ops.noise_reg(tab, flat, grad=grad, scale=1e5, accumulate=True)))
            t["noise_normalize"].append(device_ms(lambda: ops.noise_normalize(tab, flat)))
        res[f"passes_B{B}"] = dict(gz_bytes=nbytes, **{k: dict(ms=round(median(v), 4), rounds=[round(q, 4) for q in v]) for k, v in t.items()})
        print(f"noise passes alone, B = {B} ({'a map per row' if B > 1 else 'shared maps'}), g_z of all layers {nbytes / 1e9:.3f} GB: "
              + ", ".join(f"{k} {median(v):.4f} ms" for k, v in t.items()), flush=True)
    print(json.dumps(res))


def bench_compare_encoders():
    batches = [int(v) for v in a.batches.split(",")]
    models = {enc: build_models_v2(2, a.img_size, a.start_features, a.dtype, seed=0, encoder=enc) for enc in ("blur", "be")}
    G = models["blur"][0]
    with torch.no_grad():
        imgs = G.synthesis(torch.randn(max(batches + [1]), G.synthesis.num_layers, 512, device="cuda"))["image"].detach().clamp(-1, 1).contiguous()
    runs = {}
    for name, B, ind in [("B1_coupled", 1, False)] + [(f"B{B}_independent", B, True) for B in batches]:
        for enc, (Gm, E, LP) in models.items():
            st = LatentEmbedStep(Gm, E, LP, mode="W", generator="sg2", independent=ind)
            st.begin_image(imgs[:B].contiguous())
            st.capture(imgs[:B].contiguous(), warmup=1)
            for _ in range(3):
                st.replay()
            runs[f"{name}_{enc}"] = (st, B)
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name, (st, B) in runs.items():
            ms[name].append(timed(st.replay, a.iters))
    for name, (st, B) in runs.items():
        m = median(ms[name])
        res[name] = dict(ms_per_iteration=round(m, 3), ms_per_image_iteration=round(m / B, 3), rounds=[round(v, 3) for v in ms[name]])
        print(f"embedding_v2 W replay, StyleGAN2-{a.img_size}, {a.dtype}, {name}: {m:.2f} ms/iteration, {m / B:.2f} ms/image-iteration", flush=True)
    print(json.dumps(res))


def bench_last_stage():
    """Synthetic operands of block 0's last stage (conv_1's data gradient g_y1, the FromRGB output x0, the pooled skip gradient)."""
    from dge_amd import ops
    R_, C = a.img_size, a.start_features
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    for B in [int(v) for v in a.batches.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(B)
        rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
        gy, x0, extra = rn(B, R_, R_, C).to(dt), rn(B, R_, R_, C).to(dt), rn(B, R_ // 2, R_ // 2, C).to(dt)
        coef = (rn(B, C, 2), rn(B, 2 * C), torch.cat((rn(B, C), rn(B, C).abs() + 0.5), 1), rn(B, C).abs() + 0.5, rn(B, C), R_ * R_)
        w, img = rn(C, 3, 1, 1), rn(B, 3, R_, R_)
        kw = dict(extra=extra, extra_pool=True, extra_scale=0.25)

        def composed(params):
            gx0 = ops.in_bwd(gy, x0, coef, **kw)
            ops.fromrgb_dgrad(gx0, x0, w)
            if params:
                ops.fromrgb_bwd(gx0, x0, img, planar=True)
        cfg = {"frozen_fused": lambda: ops.in_bwd_fromrgb_img(gy, x0, coef, w, None, **kw), "frozen_composed": lambda: composed(False),
               "trained_fused": lambda: ops.in_bwd_fromrgb_img(gy, x0, coef, w, img, **kw), "trained_composed": lambda: composed(True)}
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


if a.optimize_noise:
    bench_noise()
    sys.exit(0)
if a.space == "z":
    bench_space_z()
    sys.exit(0)
if a.independent:
    bench_independent()
    sys.exit(0)
if a.compare_encoders:
    bench_compare_encoders()
    sys.exit(0)
if a.last_stage:
    bench_last_stage()
    sys.exit(0)
for mode in ("W", "E"):
    G, E, LP = build_models_v2(2, a.img_size, a.start_features, a.dtype, seed=0, encoder=a.encoder)
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
        print(f"embedding_v2 loop, StyleGAN2-{a.img_size} + {ENC_NAME[a.encoder]}, batch 1, {a.dtype}, mode {mode}, {launch}: {dt * 1e3:.2f} ms/iteration",
              flush=True)
        del st
print(json.dumps(res))
