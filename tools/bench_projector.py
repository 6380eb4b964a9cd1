"""ms/iteration of StyleGAN2's projector (dge_amd.projector.ProjectorStep) - dev/bench tool.  StyleGAN2-1024, random-init weights,
seeded stand-in LPIPS, one process.  Configurations alternate round by round; medians over --rounds rounds with the round spread
(max - min).
  * the iteration: batch 1 eager, batch 1 hipGraph replay, batch 8 replay (host clock around --iters iterations that end in a
    device synchronise);
  * the optimiser alone: dge_adam_multi over the parameter sets of batch 1 and batch 8 ([w, all noise maps]) against
    torch.optim.Adam on the same tensors (device events around 10 x --iters steps, eager launches: a step of tens of
    microseconds needs the longer window).
    python tools/bench_projector.py [--img-size 1024] [--dtype bf16] [--batches 1,8] [--iters 20] [--rounds 5]
  * --mask: only the masked against the unmasked iteration (README, "Masked projection"): hipGraph replay at every batch of
    --batches, a soft-edged half-plane mask, the two alternating round by round in one process; the difference of the medians
    is what the mask costs per iteration (one more f32 plane read in each prep, one m_k read per head, six head launches for
    five).
  * --styles: only the S iteration (StyleProjectorStep: the StyleSpace codes and the maps under Adam; README, "StyleSpace codes")
    against the W iteration, hipGraph replay at every batch of --batches, the two alternating round by round in one process.
    The S iteration drops dge_w_broadcast (and the dge_randn draw in front of it), dge_linear_rows and the contraction of the
    style gradients with the style weights, and steps 9088 floats per image for 512."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd  # noqa: F401
from dge_amd import ops
from dge_amd.custom_adam import Adam
from dge_amd.lpips import LPIPS
from dge_amd.projector import ProjectorStep, StyleProjectorStep

ap = argparse.ArgumentParser()
ap.add_argument("--img-size", type=int, default=1024); ap.add_argument("--dtype", default="bf16")
ap.add_argument("--fmaps-base", type=int, default=None); ap.add_argument("--fmaps-max", type=int, default=None)
ap.add_argument("--batches", default="1,8"); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--w-avg-samples", type=int, default=10000)
ap.add_argument("--mask", action="store_true", help="time the masked against the unmasked replay and nothing else")
ap.add_argument("--styles", action="store_true", help="time the S iteration against the W iteration (replay) and nothing else")
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_projector needs the GPU"
res = {}


def timed(run, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def device_ms(run, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def report(title, ms, per=None):
    for name, v in ms.items():
        m, spread = median(v), max(v) - min(v)
        res[name] = dict(ms=round(m, 4), spread=round(spread, 4), rounds=[round(q, 4) for q in v])
        extra = f", {m / per[name]:.3f} ms/image-iteration" if per else ""
        print(f"{title}, {name}: {m:.3f} ms (spread {spread:.3f}){extra}", flush=True)


torch.manual_seed(0)
kw = {k: v for k, v in (("fmaps_base", a.fmaps_base), ("fmaps_max", a.fmaps_max)) if v is not None}
G = dge_amd.StyleGAN2Generator(a.img_size, compute_dtype=a.dtype, **kw).cuda()
G.eval()
LP = LPIPS(compute_dtype=a.dtype).cuda()
batches = [int(v) for v in a.batches.split(",")]
with torch.no_grad():
    imgs = G.synthesis(torch.randn(max(batches), G.num_layers, 512, device="cuda"))["image"].detach().float().clamp(-1, 1).contiguous()

# ---- --mask: the masked against the unmasked replay
if a.mask:
    runs, per = {}, {}
    R = a.img_size
    ramp = ((R * 0.625 - torch.arange(R, dtype=torch.float32, device="cuda")) / (R / 4)).clamp(0, 1)
    for B in batches:
        x = imgs[:B].contiguous()
        m = ramp.view(1, 1, 1, R).expand(B, 1, R, R).contiguous()
        for name, mask in (("plain", None), ("masked", m)):
            st = ProjectorStep(G, LP, w_avg_samples=a.w_avg_samples)
            st.begin_image(x, mask=mask)
            st.capture(x, warmup=1)
            for _ in range(3):
                st.replay()
            runs[f"B{B}_{name}"], per[f"B{B}_{name}"] = st.replay, B
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name, run in runs.items():
            ms[name].append(timed(run, a.iters))
    report(f"projector replay with and without a mask, StyleGAN2-{a.img_size}, {a.dtype}", ms, per)
    for B in batches:
        d = res[f"B{B}_masked"]["ms"] - res[f"B{B}_plain"]["ms"]
        res[f"B{B}_mask_cost_ms"] = round(d, 4)
        print(f"B{B}: the mask costs {d:+.3f} ms per iteration ({100 * d / res[f'B{B}_plain']['ms']:+.2f} %)", flush=True)
    print(json.dumps(res))
    sys.exit(0)

# ---- --styles: the S iteration against the W iteration
if a.styles:
    runs, per = {}, {}
    for B in batches:
        x = imgs[:B].contiguous()
        st = ProjectorStep(G, LP, w_avg_samples=a.w_avg_samples)
        st.begin_image(x)
        st.capture(x, warmup=1)
        sst = StyleProjectorStep(G, LP)
        sst.begin_image(x, st.result()[1])          # (maps of its own: the two replays alternate and must not share state)
        sst.capture(x, warmup=1)
        for name, run in (("W", st.replay), ("S", sst.replay)):
            for _ in range(3):
                run()
            runs[f"B{B}_{name}"], per[f"B{B}_{name}"] = run, B
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name, run in runs.items():
            ms[name].append(timed(run, a.iters))
    report(f"projector replay, W iteration and S iteration, StyleGAN2-{a.img_size}, {a.dtype}", ms, per)
    for B in batches:
        d = res[f"B{B}_S"]["ms"] - res[f"B{B}_W"]["ms"]
        res[f"B{B}_S_minus_W_ms"] = round(d, 4)
        print(f"B{B}: the S iteration takes {d:+.3f} ms against the W iteration ({100 * d / res[f'B{B}_W']['ms']:+.2f} %); "
              f"round spreads W {res[f'B{B}_W']['spread']:.3f}, S {res[f'B{B}_S']['spread']:.3f}", flush=True)
    print(json.dumps(res))
    sys.exit(0)

# ---- the iteration
runs, per = {}, {}
for B in batches:
    for launch in (("eager", "replay") if B == 1 else ("replay",)):
        st = ProjectorStep(G, LP, w_avg_samples=a.w_avg_samples)
        x = imgs[:B].contiguous()
        st.begin_image(x)
        if launch == "replay":
            st.capture(x, warmup=1)
            run = st.replay
        else:
            run = (lambda st=st, x=x: st.step(x))
        for _ in range(3):
            run()
        runs[f"B{B}_{launch}"], per[f"B{B}_{launch}"] = run, B
ms = {k: [] for k in runs}
for _ in range(a.rounds):
    for name, run in runs.items():
        ms[name].append(timed(run, a.iters))
report(f"projector iteration, StyleGAN2-{a.img_size}, {a.dtype}", ms, per)
runs.clear()

# ---- the optimiser alone, on the parameter sets of the step
S = G.synthesis
sides = [getattr(S, f"layer{i}").res for i in range(S.num_layers - 1)]
opts = {}
for B in batches:
    shapes = [(B, 512), (B * sum(r * r for r in sides),)]
    for name, cls in (("dge_adam_multi", Adam), ("torch_adam", torch.optim.Adam)):
        ps = [torch.randn(s, device="cuda").requires_grad_(True) for s in shapes]
        for p in ps:
            p.grad = torch.randn_like(p)
        opt = cls(ps, lr=0.1, betas=(0.9, 0.999), eps=1e-8)
        for _ in range(3):
            opt.step()
        opts[f"adam_B{B}_{name}"] = opt.step
    res[f"adam_B{B}_floats"] = sum(int(torch.tensor(s).prod()) for s in shapes)
ms = {k: [] for k in opts}
for _ in range(a.rounds):
    for name, step in opts.items():
        ms[name].append(device_ms(step, 10 * a.iters))
report("Adam step over [w, noise maps]", ms)
print(json.dumps(res))
