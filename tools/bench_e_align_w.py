"""ms/iteration of the noise-free W-space training loop (dge_amd.e_align_w: scripts 3 and 2, eager launches) with the heads of
E_Blur_W / E_Blur_W_2 run two ways in the same process, alternating round by round:

  grouped   one dge_heads_rows_fwd launch in the forward, one dge_heads_rows_bwd call (two launches) in each backward
  composed  the per-head form E_Blur uses: dge_linear per head + torch.stack in the forward; per head and backward pass the row
            sum (two-row heads), dge_linear_t and dge_dense_wgrad

and the head launches' share: the same head calls alone (one forward, two backward passes), back to back on the encoder's own
table, timed with device events, over the iteration time.  The composed form lives here only (--heads composed runs it alone).
Random-init weights, seeded stand-in LPIPS - dev/bench tool.
    python tools/bench_e_align_w.py [--configs sg1-256 sg1-1024] [--variants w w_2] [--batches 2 8] [--rounds 5] [--iters 4]
                                    [--heads both|grouped|composed] [--dtype bf16]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dge_amd  # noqa: F401
from dge_amd import ops
from dge_amd.autograd_encblur import heads_rows_layout

CONFIGS = {"sg1-256": (256, 64), "sg1-1024": (1024, 16)}       # name -> (img_size, start_features)
GROUPED = (ops.heads_rows_fwd, ops.heads_rows_bwd)


def composed_heads(E):
    """(fwd, bwd) with the signatures of ops.heads_rows_fwd / heads_rows_bwd, built from ops.linear, linear_t, dense_wgrad and
    torch.stack on the encoder's own modules and flat-buffer layout."""
    L = E.layer_count

    def heads(B, dev):
        lay = heads_rows_layout(E, B, dev)
        out = []
        for name, slot, woff, boff, I in lay["items"]:
            blk, mod = name.split(".")[1], name.split(".")[2]
            j = int(blk)
            rows = [2 * (L - 1 - j) + r for r in E.w_rows[mod]]
            out.append((getattr(E.decode_block[j], mod), lay["slots"][slot][0], woff, boff, I, rows))
        return lay, out

    def fwd(tab, n, musig_all, w):
        B = w.shape[0]
        _, hs = heads(B, w.device)
        by_row = [None] * w.shape[1]
        for lin, so, _, _, I, rows in hs:
            y = ops.linear(musig_all[so:so + B * I].view(B, I), lin.weight.detach(), lin.bias.detach())
            for r in rows:
                by_row[r] = y
        w.copy_(torch.stack(by_row, dim=1))
        return w

    def bwd(tab, n, max_I, g, musig_all, gms_all, gw_all=None, gb_all=None):
        B = g.shape[0]
        lay, hs = heads(B, g.device)
        O = lay["O"]
        for lin, so, woff, boff, I, rows in hs:
            gl = g[:, rows[0]] if len(rows) == 1 else g[:, rows[0]] + g[:, rows[1]]
            ops.linear_t(gl, lin.weight.detach(), gms_all[so:so + B * I].view(B, I))
            if gw_all is not None:
                ops.dense_wgrad(gl, musig_all[so:so + B * I].view(B, I), gw_all[woff:woff + O * I].view(O, I), gb_all[boff:boff + O])
        return gms_all
    return fwd, bwd


def use(form):
    ops.heads_rows_fwd, ops.heads_rows_bwd = form


def _events(fn, iters):
    """mean time per call between two device events around `iters` calls (launch gaps the host leaves are part of it)"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3 / iters


def heads_alone(E, B, form, rounds, iters=50):
    """seconds for the head calls of one iteration (one forward, two parameter backward passes) alone: median over rounds"""
    dev = next(E.parameters()).device
    lay = heads_rows_layout(E, B, dev)
    musig = torch.randn(lay["total_m"], device=dev)
    w = torch.empty((B, 2 * E.layer_count, lay["O"]), device=dev)
    g = torch.randn_like(w)
    gms = torch.empty_like(musig)
    gw, gb = torch.empty(lay["total_w"], device=dev), torch.empty(lay["n"] * lay["O"], device=dev)
    fwd, bwd = form

    def calls():
        fwd(lay["tab"], lay["n"], musig, w)
        for _ in range(2):
            bwd(lay["tab"], lay["n"], lay["max_I"], g, musig, gms, gw, gb)
    _events(calls, 5)
    return sorted(_events(calls, iters) for _ in range(rounds))[rounds // 2]


def main():
    from dge_amd.e_align_w import EAlignWStep, build_models_w
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS)); ap.add_argument("--variants", nargs="+", default=["w", "w_2"])
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8]); ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--heads", choices=["both", "grouped", "composed"], default="both"); ap.add_argument("--dtype", default="bf16")
    a = ap.parse_args()
    res = {}
    for name in a.configs:
        size, startf = CONFIGS[name]
        for variant in a.variants:
            for B in a.batches:
                Gs, Gm, E, LP = build_models_w(variant, size, startf, a.dtype)
                st = EAlignWStep(Gs, Gm, E, LP, batch_size=B)
                forms = {"grouped": GROUPED, "composed": composed_heads(E)}
                if a.heads != "both":
                    forms = {a.heads: forms[a.heads]}
                it = [0]

                def step():
                    st.step(it[0]); it[0] += 1
                try:
                    for f in forms.values():            # warm every form (code objects, allocator) before the timed rounds
                        use(f)
                        for _ in range(a.warmup):
                            step()
                    torch.cuda.synchronize()
                    ts = {k: [] for k in forms}
                    for _ in range(a.rounds):           # same process, alternating
                        for k, f in forms.items():
                            use(f)
                            ts[k].append(_events(step, a.iters))
                    for k, f in forms.items():
                        ms = sorted(ts[k])[len(ts[k]) // 2] * 1e3
                        hd = heads_alone(E, B, f, a.rounds) * 1e3
                        key = f"{name}_{variant}_b{B}_{k}"
                        res[key + "_ms"], res[key + "_heads_ms"], res[key + "_heads_share"] = round(ms, 2), round(hd, 3), round(hd / ms, 4)
                        print(f"{name} E_Blur_{variant.upper()} batch {B} {a.dtype} heads {k}: {ms:.2f} ms/iteration (median of {a.rounds} x {a.iters}; "
                              f"min {min(ts[k]) * 1e3:.2f}, max {max(ts[k]) * 1e3:.2f}), head calls alone {hd:.3f} ms = {100 * hd / ms:.2f} %", flush=True)
                finally:
                    use(GROUPED)
                del st, Gs, Gm, E, LP
                torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
