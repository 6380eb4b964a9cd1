"""ms/step of the Z-space encoder training loop (dge_amd.e_align_z: StyleGAN1 FFHQ-1024 + E_Blur_Z, eager) and an A/B of the fused
mapping backward (dge_mapping_bwd, one launch) against the same math built from existing ops (8 dge_linear_t plus elementwise
work), both on the activations a per-layer forward saved, timed with device events in the same process - dev/bench tool.
Random-init weights, seeded stand-in LPIPS.
    python tools/bench_e_align_z.py [--img-size 1024] [--batches 2 8] [--iters 10] [--dtype bf16]
--mapping-only: the mapping adjoint alone on a 8 x 512 mapping network with L W+ rows - dge_mapping_bwd on saved activations (one
launch, one workgroup per sample), dge_mapping_bwd_wide (one chip-wide launch per layer) and the dge_linear_t composition - one
process, the three alternating round by round, medians of --rounds rounds with the round spread (max - min).
    python tools/bench_e_align_z.py --mapping-only [--batches 1 2 4 8] [--rows 18] [--rounds 5]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd  # noqa: F401
from dge_amd import ops


def composed_mapping_bwd(M, z, g, coefs=None, acts=None, eps=1e-8):
    """dz of sum(g * Mapping(z)) from existing ops: the lerp / broadcast adjoint, per layer the leaky-relu mask and dge_linear_t,
    then the pixel-norm backward.  `acts`: the layer outputs of the forward (Mapping.activations).  The reference for
    tests/test_e_align_z_gpu.py and the B side of the A/B below."""
    acts = M.activations(z) if acts is None else acts
    gy = (g * coefs.view(1, -1, 1)).sum(1) if coefs is not None else g.sum(1)
    for l in range(len(acts) - 1, -1, -1):
        W = getattr(M, "block_%d" % (l + 1)).fc.weight.detach()
        gpre = torch.where(acts[l] > 0, gy, 0.2 * gy)
        gx = torch.empty((gy.shape[0], W.shape[1]), dtype=torch.float32, device=gy.device)
        ops.linear_t(gpre, W, gx)
        gy = gx
    r = torch.rsqrt(z.pow(2).mean(1, keepdim=True) + eps)
    return r * gy - z * (r ** 3) * (gy * z).sum(1, keepdim=True) / z.shape[1]


def _time(fn, iters):
    """mean time per call between two device events around `iters` calls (launch gaps the host leaves are part of it)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3 / iters


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def mapping_only(a):
    from dge_amd.stylegan1 import Mapping
    torch.manual_seed(0)
    res = {}
    Gm = Mapping(num_layers=a.rows).cuda()
    for B in a.batches:
        z = torch.randn(B, 512, device="cuda")
        g = torch.randn(B, a.rows, 512, device="cuda")
        coefs = torch.where(torch.arange(a.rows) < a.rows // 2, 0.7, 1.0).float().cuda()
        acts = Gm.activations(z)
        work = torch.empty(ops.mapping_bwd_work_bytes(B), dtype=torch.uint8, device="cuda")
        cfg = {"one_launch": lambda: ops.mapping_bwd(z, Gm.chain(), g, coefs=coefs, acts=acts),
               "wide": lambda: ops.mapping_bwd(z, Gm.chain(), g, coefs=coefs, acts=acts, wide=True, work=work),
               "composed": lambda: composed_mapping_bwd(Gm, z, g, coefs, acts=acts)}
        t = {k: [] for k in cfg}
        for _ in range(a.rounds):
            for k, f in cfg.items():
                t[k].append(_time(f, 200) * 1e6)
        res[f"B{B}"] = {k: dict(us=round(_median(v), 1), spread=round(max(v) - min(v), 1), rounds=[round(q, 1) for q in v]) for k, v in t.items()}
        print(f"mapping adjoint alone, B = {B}, L = {a.rows} (us per call, 200 back-to-back calls between two device events; median of "
              f"{a.rounds} rounds, spread): " + ", ".join(f"{k} {_median(v):.1f} ({max(v) - min(v):.1f})" for k, v in t.items()), flush=True)
    print(json.dumps(res))


def main():
    from dge_amd.e_align_z import EAlignZStep, build_models_z
    ap = argparse.ArgumentParser()
    ap.add_argument("--img-size", type=int, default=1024); ap.add_argument("--start-features", type=int, default=16)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8]); ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--mapping-only", action="store_true"); ap.add_argument("--rows", type=int, default=18)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.mapping_only:
        return mapping_only(a)
    res = {}
    for B in a.batches:
        Gs, Gm, E, LP = build_models_z(a.img_size, a.start_features, a.dtype)
        st = EAlignZStep(Gs, Gm, E, LP, batch_size=B)
        it = [0]

        def step():
            st.step(it[0]); it[0] += 1
        dt = _time(step, a.iters)
        res[f"step_ms_b{B}"] = round(dt * 1e3, 2)
        print(f"e_align_z step, StyleGAN1-{a.img_size} + E_Blur_Z, batch {B}, {a.dtype}, eager: {dt * 1e3:.2f} ms/step", flush=True)
        # mapping backward A/B on this model's mapping network
        L = 2 * Gs.layer_count
        z = torch.randn(B, 512, device="cuda")
        g = torch.randn(B, L, 512, device="cuda")
        coefs = Gm.truncation(st.gen.coefs, z.device, 512)[1]
        acts = Gm.activations(z)                 # saved by MappingFunction.forward in the step
        fused = _time(lambda: ops.mapping_bwd(z, Gm.chain(), g, coefs=coefs, acts=acts), 200)
        recomp = _time(lambda: ops.mapping_bwd(z, Gm.chain(), g, coefs=coefs), 200)
        work = torch.empty(ops.mapping_bwd_work_bytes(B), dtype=torch.uint8, device="cuda")
        wide = _time(lambda: ops.mapping_bwd(z, Gm.chain(), g, coefs=coefs, acts=acts, wide=True, work=work), 200)
        comp = _time(lambda: composed_mapping_bwd(Gm, z, g, coefs, acts=acts), 200)
        ref = composed_mapping_bwd(Gm, z, g, coefs, acts=acts)
        err = ((ops.mapping_bwd(z, Gm.chain(), g, coefs=coefs, acts=acts) - ref).abs().max() / ref.abs().max()).item()
        res[f"mapping_bwd_fused_us_b{B}"] = round(fused * 1e6, 1)
        res[f"mapping_bwd_fused_recompute_us_b{B}"] = round(recomp * 1e6, 1)
        res[f"mapping_bwd_composed_us_b{B}"] = round(comp * 1e6, 1)
        res[f"mapping_bwd_wide_us_b{B}"] = round(wide * 1e6, 1)
        print(f"mapping backward, batch {B} (activations saved by the forward): fused {fused * 1e6:.1f} us, wide {wide * 1e6:.1f} us, "
              f"composed {comp * 1e6:.1f} us; "
              f"fused with the forward recomputed inside {recomp * 1e6:.1f} us; max rel diff {err:.2e}", flush=True)
        del st, Gs, Gm, E, LP
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
