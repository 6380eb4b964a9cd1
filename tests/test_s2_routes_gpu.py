"""Which launcher every layer of the StyleGAN2 synthesis forward and of its hand-written backward runs on (s2_conv.forward_route /
dgrad_route), pinned as literals: one synthesis forward + backward per case with spies on the ops launchers; per launch, in call
order, the launcher, its mode flags (up, in_s2d, in_t2d, dgrad), whether `prep` (the tail backward of the layer below) was passed,
and the kernel the library then launched (`last_kernel()`); and s2_conv.dgrad_takes_prep against what the backward then did, for
every layer walked.  The test judges routes, not numbers: the weights are whatever the constructor drew.

Cases: bf16 in atomics mode, bf16 in deterministic mode, f32 in atomics mode.  The same spies on the default 1024^2 generator at
batch 8 show, per case, no (launcher, flags) pair that the generators below do not show too - no route appears at 1024^2 only.
Which layer stands for which route of that generator (its layer in brackets):

  S = 64^2, fmaps_base 2048, fmaps_max 128 (the generator of tests/golden/s2_small.npz), batch 2; bf16 cases and f32
      forward   layers 1, 3: conv2d(up), the folded form [1, 3];  layer 5 (128 -> 64 on 16^2): up_pp [5 .. 13];  layer 7
                (64 -> 32): upconv_fir [15];  even layers: conv2d [0 .. 6, 14, 16];  f32: layers 5, 7 upconv_fir [5 .. 15]
      backward  bf16 atomics: layer 7: up_dgrad_stream with prep [15];  layers 1, 3, 5: conv2d(in_s2d) with prep;  even
                layers: conv2d with prep [16, 14, 6 .. 2], layer 0 without [0]
                bf16 deterministic: layer 7: conv2d(in_t2d), the phase form on conv2d [7, 9, 11];  layers 5, 3, 1: conv2d(in_s2d)
                [15, 13, 5, 3, 1];  even layers: conv2d;  no prep, modconv_bwd_prep before every launch
                f32 atomics: layer 7: conv2d(in_t2d) with prep [7, 9, 11];  layers 5, 3, 1 (128 channels in): conv2d(in_s2d)
                with prep [13, 5, 3, 1]
  W = 512^2, fmaps_base 32768, fmaps_max 512 (the 1024^2 generator without its top two layers), batch 3; bf16 cases
      forward   layers 10, 12: conv_pp [8, 10, 12];  layers 5 .. 13 (odd): up_pp;  layers 1, 3: conv2d(up)
      backward  bf16 atomics: layers 12, 10: conv_pp(dgrad) [12, 10, 8];  layer 13 (128 -> 64, 256^2 grid): conv_pp(dgrad,
                in_s2d) [13];  layer 11 (256 -> 128, 128^2 grid): conv_pp(dgrad, in_t2d) [11, 9];  layer 9: conv2d(in_t2d) (too
                few tiles for conv_pp at batch 3);  layers 7, 5, 3, 1: up_dgrad_small [7, 5, 3, 1];  the other even layers: conv2d
                bf16 deterministic: layers 7, 9, 11: conv2d(in_t2d);  13, 5, 3, 1: conv2d(in_s2d);  even layers: conv2d
  N = 64^2, fmaps_base 2048, fmaps_max 64, batch 2; f32
      forward   layers 5, 7: upconv_fir;  layers 1, 3: conv2d(up);  even layers: conv2d
      backward  layer 7 (grid 32^2): conv2d(in_t2d) with prep;  layers 5, 3, 1 (64 channels in: narrow, and below the grids of
                the phase form): conv2d(in_s2d) WITHOUT prep [15], so layers 4, 2, 0 are atomics-mode layers whose tail backward
                runs as a pass of its own, modconv_bwd_prep [14 below 15]"""
import pytest
import torch

pytestmark = pytest.mark.gpu

GENERATORS = {"S": dict(res=64, fmaps_base=2048, fmaps_max=128, B=2), "W": dict(res=512, fmaps_base=32768, fmaps_max=512, B=3),
              "N": dict(res=64, fmaps_base=2048, fmaps_max=64, B=2)}
CASES = {"bf16_atomics": ("bf16", False, ("S", "W")), "bf16_det": ("bf16", True, ("S", "W")), "f32_atomics": ("f32", False, ("N", "S"))}
LAUNCHERS = ("conv2d", "conv_pp", "up_pp", "upconv_fir", "up_dgrad_stream", "up_dgrad_small")
FLAGS = ("up", "in_s2d", "in_t2d", "dgrad", "prep")


def walk(G, B, monkeypatch):
    """One synthesis forward + backward of G at batch B under the spies -> (forward records, backward records); a record is
    "launcher[flags] kernel", and "modconv_bwd_prep" for a tail backward that ran as a pass of its own."""
    import dge_amd
    from dge_amd import ops
    log = []

    def spy(name):
        real = getattr(ops, name)

        def f(*a, **k):
            out = real(*a, **k)
            flags = ",".join(n for n in FLAGS if k.get(n) is not None and k.get(n) is not False)
            log.append(f"{name}[{flags}] {dge_amd._lib.last_kernel()}")
            return out
        return f

    real_prep = ops.modconv_bwd_prep

    def spy_prep(*a, **k):
        log.append("modconv_bwd_prep")
        return real_prep(*a, **k)

    with monkeypatch.context() as m:
        for name in LAUNCHERS:
            m.setattr(ops, name, spy(name))
        m.setattr(ops, "modconv_bwd_prep", spy_prep)
        torch.manual_seed(5)
        wp = torch.randn(B, G.synthesis.num_layers, 512, device="cuda").requires_grad_(True)
        img = G.synthesis(wp)["image"]
        fwd = list(log)
        del log[:]
        (img * torch.randn_like(img)).sum().backward()
    torch.cuda.synchronize()
    assert wp.grad is not None and bool(torch.isfinite(wp.grad).all())
    return fwd, list(log)


def make_generator(res, fmaps_base, fmaps_max, dtype):
    import dge_amd
    torch.manual_seed(3)
    return dge_amd.StyleGAN2Generator(res, fmaps_base=fmaps_base, fmaps_max=fmaps_max, compute_dtype=dtype).cuda()


@pytest.fixture(scope="module")
def generators():
    made = {}

    def get(name, dtype):
        if (name, dtype) not in made:
            g = GENERATORS[name]
            made[(name, dtype)] = make_generator(g["res"], g["fmaps_base"], g["fmaps_max"], dtype)
        return made[(name, dtype)]
    yield get
    made.clear()


def run_case(case, get, monkeypatch):
    """{generator name: (forward records, backward records)} of a case, with the takes_prep check on every layer walked."""
    from dge_amd import ops, s2_conv
    dtype, det, names = CASES[case]
    was = ops.is_deterministic()
    ops.set_deterministic(det)
    try:
        got = {}
        for name in names:
            G, B = get(name, dtype), GENERATORS[name]["B"]
            fwd, bwd = walk(G, B, monkeypatch)
            nl = G.synthesis.num_layers
            launches = [r for r in bwd if r != "modconv_bwd_prep"]              # one data-gradient launch per layer, top layer first
            assert len(fwd) == nl - 1 and len(launches) == nl - 1, (case, name, fwd, bwd)
            dt = ops.BF16 if dtype == "bf16" else ops.F32
            for i, rec in zip(range(nl - 2, -1, -1), launches):
                L = getattr(G.synthesis, f"layer{i}")
                took = "prep" in rec.split("]")[0].split("[")[1].split(",")
                # (the backward passes `prep` in atomics mode and where a layer below exists)
                assert took == bool((not det) and i >= 1 and s2_conv.dgrad_takes_prep(L, B, dt)), (case, name, i, rec)
            got[name] = (fwd, bwd)
        return got
    finally:
        ops.set_deterministic(was)


# Recorded at the commit before s2_conv.dgrad_route / forward_route existed, with only this file added; layer order: forward 0 .. top,
# backward top .. 0 ("modconv_bwd_prep" precedes the launch of the layer whose tail it is).
WALKS = {
    ("bf16_atomics", "S"): dict(
        fwd=[
            "conv2d[] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "conv2d[up] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "conv2d[] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "conv2d[up] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "conv2d[] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "up_pp[] up_s4<bf16,8,32,32>",
            "conv2d[] conv_igemm<bf16,8,8,64,64,3,2,2>",
            "upconv_fir[] upconv_fir<bf16>",
            "conv2d[] conv_igemm<bf16,8,16,32,32,3,4,1>",
        ],
        bwd=[
            "conv2d[prep] conv_igemm<bf16,8,16,32,32,3,4,1>+prep",
            "up_dgrad_stream[prep] upconv_stream_bwd<bf16,64,32>+prep",
            "conv2d[prep] conv_igemm<bf16,8,8,64,64,3,2,2>+prep",
            "conv2d[in_s2d,prep] conv_igemm<bf16,8,8,64,64,3,2,2>+prep",
            "conv2d[prep] conv_igemm<bf16,8,8,64,128,3,2,2>+prep",
            "conv2d[in_s2d,prep] conv_igemm<bf16,8,8,64,128,3,2,2>+prep",
            "conv2d[prep] conv_igemm<bf16,8,8,64,128,3,2,2>+prep",
            "conv2d[in_s2d,prep] conv_igemm<bf16,8,8,64,128,3,2,2>+prep",
            "conv2d[] conv_igemm<bf16,8,8,64,128,3,2,2>",
        ],
    ),
    ("bf16_atomics", "W"): dict(
        fwd=[
            "conv2d[] conv_small<bf16,8,8,64,512>",
            "conv2d[up] conv_small<bf16,8,8,64,512>",
            "conv2d[] conv_small<bf16,8,8,64,512>",
            "conv2d[up] conv_small<bf16,8,8,64,512>",
            "conv2d[] conv_small<bf16,8,8,64,512>",
            "up_pp[] up_s4<bf16,8,32,32>",
            "conv2d[] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "up_pp[] up_s4<bf16,8,32,32>",
            "conv2d[] conv_igemm<bf16,16,16,64,32,3,4,1>+tr",
            "up_pp[] up_s4<bf16,8,32,32>",
            "conv_pp[] conv_pp<bf16,16,32,128>",
            "up_pp[] up_s4<bf16,8,32,32>",
            "conv_pp[] conv_pp<bf16,16,32,128>",
            "up_pp[] up_s4<bf16,8,32,32>",
            "conv2d[] conv_stream<bf16,64,64,gen_rgb>",
        ],
        bwd=[
            "conv2d[prep] conv_stream<bf16,64,64,dot_prep>",
            "conv_pp[in_s2d,dgrad,prep] conv_pp<bf16,16,32,128>+dg+s2d+prep",
            "conv_pp[dgrad,prep] conv_pp<bf16,16,32,128>+dg+prep",
            "conv_pp[in_t2d,dgrad,prep] conv_pp<bf16,16,32,128>+dg+t2d+prep",
            "conv_pp[dgrad,prep] conv_pp<bf16,16,32,128>+dg+prep",
            "conv2d[in_t2d,prep] conv_igemm<bf16,16,16,64,32,3,4,1>+t2d+prep",
            "conv2d[prep] conv_igemm<bf16,16,16,64,32,3,4,1>+prep",
            "up_dgrad_small[prep] conv_small<bf16,8,8,64,512>+t2d+prep",
            "conv2d[prep] conv_igemm<bf16,8,8,64,128,3,2,2>+prep",
            "up_dgrad_small[prep] conv_small<bf16,8,8,64,512>+t2d+prep",
            "conv2d[prep] conv_small<bf16,8,8,64,512>+prep",
            "up_dgrad_small[prep] conv_small<bf16,8,8,64,512>+t2d+prep",
            "conv2d[prep] conv_small<bf16,8,8,64,512>+prep",
            "up_dgrad_small[prep] conv_small<bf16,8,8,64,512>+t2d+prep",
            "conv2d[] conv_small<bf16,8,8,64,512>",
        ],
    ),
    ("bf16_det", "S"): dict(
        fwd=[
            "conv2d[] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "conv2d[up] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "conv2d[] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "conv2d[up] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "conv2d[] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "up_pp[] up_s4<bf16,8,32,32>",
            "conv2d[] conv_igemm<bf16,8,8,64,64,3,2,2>",
            "upconv_fir[] upconv_fir<bf16>",
            "conv2d[] conv_igemm<bf16,8,16,32,32,3,4,1>",
        ],
        bwd=[
            "modconv_bwd_prep",
            "conv2d[] conv_igemm<bf16,8,16,32,32,3,4,1>",
            "modconv_bwd_prep",
            "conv2d[in_t2d] conv_igemm<bf16,16,16,64,32,3,4,1>+t2d",
            "modconv_bwd_prep",
            "conv2d[] conv_igemm<bf16,8,8,64,64,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[in_s2d] conv_igemm<bf16,8,8,64,64,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[in_s2d] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[in_s2d] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[] conv_igemm<bf16,8,8,64,128,3,2,2>",
        ],
    ),
    ("bf16_det", "W"): dict(
        fwd=[
            "conv2d[] conv_small<bf16,8,8,64,512>",
            "conv2d[up] conv_small<bf16,8,8,64,512>",
            "conv2d[] conv_small<bf16,8,8,64,512>",
            "conv2d[up] conv_small<bf16,8,8,64,512>",
            "conv2d[] conv_small<bf16,8,8,64,512>",
            "up_pp[] up_s4<bf16,8,32,32>",
            "conv2d[] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "up_pp[] up_s4<bf16,8,32,32>",
            "conv2d[] conv_igemm<bf16,16,16,64,32,3,4,1>+tr",
            "up_pp[] up_s4<bf16,8,32,32>",
            "conv_pp[] conv_pp<bf16,16,32,128>",
            "up_pp[] up_s4<bf16,8,32,32>",
            "conv_pp[] conv_pp<bf16,16,32,128>",
            "up_pp[] up_s4<bf16,8,32,32>",
            "conv2d[] conv_stream<bf16,64,64,gen_rgb>",
        ],
        bwd=[
            "modconv_bwd_prep",
            "conv2d[] conv_stream<bf16,64,64,dot>",
            "modconv_bwd_prep",
            "conv2d[in_s2d] conv_igemm<bf16,16,16,128,32,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[] conv_igemm<bf16,16,16,128,32,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[in_t2d] conv_igemm<bf16,16,16,64,32,3,4,1>+t2d",
            "modconv_bwd_prep",
            "conv2d[] conv_igemm<bf16,16,16,64,32,3,4,1>",
            "modconv_bwd_prep",
            "conv2d[in_t2d] conv_igemm<bf16,16,16,64,32,3,4,1>+t2d",
            "modconv_bwd_prep",
            "conv2d[] conv_igemm<bf16,16,16,64,32,3,4,1>",
            "modconv_bwd_prep",
            "conv2d[in_t2d] conv_igemm<bf16,16,16,64,32,3,4,1>+t2d",
            "modconv_bwd_prep",
            "conv2d[] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[in_s2d] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[] conv_small<bf16,8,8,64,512>",
            "modconv_bwd_prep",
            "conv2d[in_s2d] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[] conv_small<bf16,8,8,64,512>",
            "modconv_bwd_prep",
            "conv2d[in_s2d] conv_igemm<bf16,8,8,64,128,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[] conv_small<bf16,8,8,64,512>",
        ],
    ),
    ("f32_atomics", "N"): dict(
        fwd=[
            "conv2d[] conv_igemm<f32,8,8,64,64,3,2,2>",
            "conv2d[up] conv_igemm<f32,8,8,64,64,3,2,2>",
            "conv2d[] conv_igemm<f32,8,8,64,64,3,2,2>",
            "conv2d[up] conv_igemm<f32,8,8,64,64,3,2,2>",
            "conv2d[] conv_igemm<f32,8,8,64,64,3,2,2>",
            "upconv_fir[] upconv_fir<f32>",
            "conv2d[] conv_igemm<f32,8,8,64,64,3,2,2>",
            "upconv_fir[] upconv_fir<f32>",
            "conv2d[] conv_igemm<f32,8,16,32,16,3,4,1>",
        ],
        bwd=[
            "conv2d[prep] conv_igemm<f32,8,16,32,16,3,4,1>+prep",
            "conv2d[in_t2d,prep] conv_igemm<f32,16,16,64,16,3,4,1>+t2d+prep",
            "conv2d[prep] conv_igemm<f32,8,8,64,64,3,2,2>+prep",
            "conv2d[in_s2d] conv_igemm<f32,8,8,64,64,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[prep] conv_igemm<f32,8,8,64,64,3,2,2>+prep",
            "conv2d[in_s2d] conv_igemm<f32,8,8,64,64,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[prep] conv_igemm<f32,8,8,64,64,3,2,2>+prep",
            "conv2d[in_s2d] conv_igemm<f32,8,8,64,64,3,2,2>",
            "modconv_bwd_prep",
            "conv2d[] conv_igemm<f32,8,8,64,64,3,2,2>",
        ],
    ),
    ("f32_atomics", "S"): dict(
        fwd=[
            "conv2d[] conv_igemm<f32,8,8,64,64,3,2,2>",
            "conv2d[up] conv_igemm<f32,8,8,64,64,3,2,2>",
            "conv2d[] conv_igemm<f32,8,8,64,64,3,2,2>",
            "conv2d[up] conv_igemm<f32,8,8,64,64,3,2,2>",
            "conv2d[] conv_igemm<f32,8,8,64,64,3,2,2>",
            "upconv_fir[] upconv_fir<f32>",
            "conv2d[] conv_igemm<f32,8,8,64,64,3,2,2>",
            "upconv_fir[] upconv_fir<f32>",
            "conv2d[] conv_igemm<f32,8,16,32,16,3,4,1>",
        ],
        bwd=[
            "conv2d[prep] conv_igemm<f32,8,16,32,16,3,4,1>+prep",
            "conv2d[in_t2d,prep] conv_igemm<f32,16,16,64,16,3,4,1>+t2d+prep",
            "conv2d[prep] conv_igemm<f32,8,8,64,64,3,2,2>+prep",
            "conv2d[in_s2d,prep] conv_igemm<f32,8,8,64,64,3,2,2>+prep",
            "conv2d[prep] conv_igemm<f32,8,8,64,64,3,2,2>+prep",
            "conv2d[in_s2d,prep] conv_igemm<f32,8,8,64,64,3,2,2>+prep",
            "conv2d[prep] conv_igemm<f32,8,8,64,64,3,2,2>+prep",
            "conv2d[in_s2d,prep] conv_igemm<f32,8,8,64,64,3,2,2>+prep",
            "conv2d[] conv_igemm<f32,8,8,64,64,3,2,2>",
        ],
    ),
}


@pytest.mark.nondet
@pytest.mark.parametrize("case", list(CASES))
def test_synthesis_routes_are_the_recorded_ones(case, generators, monkeypatch):
    got = run_case(case, generators, monkeypatch)
    for name, (fwd, bwd) in got.items():
        print(f"ROUTES {case} {name} fwd {fwd}")
        print(f"ROUTES {case} {name} bwd {bwd}")
    for name, (fwd, bwd) in got.items():
        want = WALKS[(case, name)]
        assert fwd == want["fwd"], (case, name, "forward")
        assert bwd == want["bwd"], (case, name, "backward")
