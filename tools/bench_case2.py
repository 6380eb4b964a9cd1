"""ms/iteration of the per-loss-update training loop (dge_amd.e_align_case2, eager launches) at StyleGAN1-256 and StyleGAN2-1024,
and an A/B of the split window-gradient kernel (dge_space_loss_bwd_split, one launch, no memset) against three single-window
dge_space_loss_bwd launches into pre-zeroed images - both paths in the same process, interleaved round by round, timed with
device events - dev/bench tool.  Random-init weights, seeded stand-in LPIPS.
    python tools/bench_case2.py [--configs sg1-256 s2-1024] [--batch 8] [--iters 10] [--dtype bf16] [--loss-only]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd  # noqa: F401
from dge_amd._lib import lib, check

CONFIGS = {"sg1-256": (1, 256, 64), "s2-1024": (2, 1024, 16)}       # name -> (mtype, img_size, start_features)


def _events(fn, iters):
    """mean time per call between two device events around `iters` calls (launch gaps the host leaves are part of it)"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3 / iters


def loss_ab(B, size, rounds=5, iters=50):
    """(split, three launches + memsets) seconds per call: medians over `rounds` alternating rounds, after a warm-up of each"""
    from dge_amd.losses import attention_windows, _pool_factor
    L = lib()
    a = torch.randn(B, 3, size, size, device="cuda")
    b = a * 0.8 + 0.2 * torch.randn_like(a)
    wins = attention_windows(size, size)
    ks = [_pool_factor(w[2]) for w in wins]
    sums = [torch.rand(8, device="cuda") + 1.0 for _ in wins]
    gps = [torch.randn(B, 3, w[2] // k, w[3] // k, device="cuda") * 1e-3 for w, k in zip(wins, ks)]
    ns = [float(B * 3 * w[2] * w[3]) for w in wins]
    outs = [torch.empty_like(a) for _ in wins]
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    wflat = (C.c_int * 12)(*[int(v) for w in wins for v in w])
    kk, nn, ww = (C.c_int * 3)(*ks), (C.c_float * 3)(*ns), (C.c_float * 3)(1.0, 5.0, 9.0)

    def split():
        check(L.dge_space_loss_bwd_split(a.data_ptr(), b.data_ptr(), ptr(sums), ptr(gps), ptr(outs), B * 3, size, size, wflat, kk, nn, ww, 3, st))

    def three():
        for i, (y0, x0, h, w) in enumerate(wins):
            outs[i].zero_()
            check(L.dge_space_loss_bwd(a.data_ptr(), b.data_ptr(), sums[i].data_ptr(), gps[i].data_ptr(), outs[i].data_ptr(), B * 3, size, size,
                                       y0, x0, h, w, ks[i], ns[i], (1.0, 5.0, 9.0)[i], 0, st))
    for fn in (split, three):
        _events(fn, 5)
    ts = {"split": [], "three": []}
    for _ in range(rounds):
        ts["split"].append(_events(split, iters))
        ts["three"].append(_events(three, iters))
    med = lambda v: sorted(v)[len(v) // 2]
    return med(ts["split"]), med(ts["three"])


def main():
    from dge_amd.e_align_case2 import Case2Step, build_models
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS)); ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--loss-only", action="store_true")
    a = ap.parse_args()
    res = {}
    for name in a.configs:
        mtype, size, startf = CONFIGS[name]
        s, t = loss_ab(a.batch, size)
        res[f"{name}_loss_split_us"], res[f"{name}_loss_three_launches_us"] = round(s * 1e6, 1), round(t * 1e6, 1)
        print(f"{name} batch {a.batch}: window gradients split kernel {s * 1e6:.1f} us, three launches + memsets {t * 1e6:.1f} us", flush=True)
        if a.loss_only:
            continue
        G, Gm, E, LP = build_models(mtype, size, startf, a.dtype)
        st = Case2Step(G, E, LP, mapping=Gm, latent_terms=("w", "c") if mtype == 1 else ("w",), latent_scale=0.01 if mtype == 1 else 1.0,
                       batch_size=a.batch)
        it = [0]

        def step():
            st.step(it[0]); it[0] += 1
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        dt = _events(step, a.iters)
        res[f"{name}_step_ms_b{a.batch}"] = round(dt * 1e3, 2)
        print(f"case-2 iteration (3 image steps + latent step), {name}, batch {a.batch}, {a.dtype}, eager: {dt * 1e3:.2f} ms", flush=True)
        del st, G, Gm, E, LP
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
