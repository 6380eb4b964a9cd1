"""The v2 inversion loop (dge_amd.embedding_v2) with E.BE - the encoder E_align trains - in E_Blur's place: two iterations of the
reference's own modules (tests/golden/embed_v2_be.npz, tools/gen_golden.py `embed_v2_be`) for StyleGAN2 x encoder fine-tuning / W+
optimisation and StyleGAN1 x encoder fine-tuning, graph replay against eager, and the full-size StyleGAN2-1024 loop.  Helpers,
assertions and bounds are those of tests/test_embed_v2_gpu.py."""
import numpy as np
import pytest
import torch

from tests.conftest import MODES, golden, meas
from tests.golden import recipe as R
from tests.test_embed_v2_gpu import begin, case_noises, l2rel, make_models, relerr
from oracle import lpips_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [("sg2", "E"), ("sg2", "W"), ("sg1", "E")]


def make_models_be(gen, cd="f32"):
    from dge_amd.encoder import BE
    G, _, LP = make_models(gen, cd)
    E = BE(startf=16, maxf=64, layer_count=5, compute_dtype=cd).cuda()
    E.load_state_dict(R.fill_encoder({k: list(v.shape) for k, v in E.state_dict().items()}, seed=71))
    return G, E, LP


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gen,opt", CASES)
def test_embed_v2_be_loop_matches_reference_run(gen, opt, mode):
    from dge_amd.embedding_v2 import LatentEmbedStep
    g = golden("embed_v2_be.npz")
    tag = f"{gen}_{opt}"
    G, E, LP = make_models_be(gen)
    st = LatentEmbedStep(G, E, LP, mode=opt, generator=gen, lr=0.005)
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    begin(st, g, gen, opt, imgs1)
    if opt == "W":
        assert relerr(st.w1, g[f"{tag}_w0"]) < 1e-3
    lt = 1e-3 if mode == "det" else 3e-3
    pnames = ["decode_block.0.conv_1.weight", "decode_block.2.inver_mod1.bias", "FromRGB.from_rgb.weight"]
    for it in range(2):
        calls = []
        orig = st.opt.step

        def spy(*a, **kw):
            if opt == "E":
                calls.append({k: p.grad.detach().clone() for k, p in E.named_parameters() if k in pnames})
            else:
                calls.append({"w1": st.w1.grad.detach().clone()})
            return orig(*a, **kw)
        st.opt.step = spy
        try:
            r = st.step(imgs1, noises=case_noises(g, tag, it))
        finally:
            st.opt.step = orig
        pre = f"{tag}_it{it}"
        e_w1 = relerr(r["w1"], g[f"{pre}_w1"])
        meas(f"embed_v2_be.{tag}.{mode}.it{it}", w1=e_w1, w1_l2=l2rel(r["w1"], g[f"{pre}_w1"]), w2=relerr(r["w2"], g[f"{pre}_w2"]))
        if opt == "W":
            assert l2rel(r["w1"], g[f"{pre}_w1"]) < 1e-3 and e_w1 < 4e-3, (it, e_w1)
        else:
            assert e_w1 < 1e-3, (it, e_w1)
        assert relerr(r["w2"], g[f"{pre}_w2"]) < (2e-3 if it == 0 else 1e-2), it
        if f"{pre}_imgs2" in g.files:
            assert relerr(r["imgs2"], g[f"{pre}_imgs2"]) < 2e-3
        assert relerr(r["const3"], g[f"{pre}_const3"]) < (2e-3 if it == 0 else 1e-2)
        if f"{pre}_const2" in g.files:
            assert relerr(r["const2"], g[f"{pre}_const2"]) < 1e-3
        else:
            assert r["const2"] is None and r["loss_c1"] is None
        info = r["info_img"].cpu().numpy()
        got = [float(r["loss_msiv"]), info[0, 0], info[1, 0], info[2, 0], float(r["loss_w"]),
               float(r["loss_c1"]) if r["loss_c1"] is not None else 0.0, float(r["norm"]), float(r["loss_mslv"])]
        ref = g[f"{pre}_losses"]
        for k, (a, b) in enumerate(zip(got, ref)):
            assert abs(a - b) <= (lt if it == 0 else 3 * lt) * abs(b) + 1e-7, (it, k, got, ref.tolist())
        for key in g.files:
            if key.startswith(f"{pre}_grad1:") or key.startswith(f"{pre}_grad2:"):
                phase = 0 if "_grad1:" in key else 1
                k = key.split(":", 1)[1]
                e = l2rel(calls[phase][k], g[key])
                meas(f"embed_v2_be.{tag}.{mode}.it{it}.grad{phase + 1}", key=k, l2=e)
                assert e < (5e-3 if phase == 0 and it == 0 else 6e-2), (it, phase, k, e)
        if opt == "E":
            ck = R.checksum({k: v.cpu() for k, v in E.state_dict().items()})
        else:
            ck = R.checksum({"w1": st.w1.detach().cpu()})
        assert abs(ck - float(g[f"{pre}_param_checksum"])) < 2e-4 * float(g[f"{pre}_param_checksum"])


def test_be_w_mode_replay_equals_eager_bitwise():
    """W mode, StyleGAN2-64 + E.BE, deterministic mode: 5 replays of the captured iteration give the bits of 5 eager iterations."""
    from dge_amd import ops
    from dge_amd.embedding_v2 import LatentEmbedStep
    g = golden("embed_v2_be.npz")
    imgs1 = torch.as_tensor(g["imgs1"]).cuda()
    w0 = torch.as_tensor(g["sg2_W_w0"])
    noises = case_noises(g, "sg2_W", 0)
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        G, E, LP = make_models_be("sg2")
        a = LatentEmbedStep(G, E, LP, mode="W", generator="sg2", lr=0.005)
        a.begin_image(imgs1, w_init=w0)
        a.opt.graph_begin(2, imgs1.device)
        wa = []
        for _ in range(5):
            a.opt.graph_advance()
            wa.append(a.step(imgs1, noises)["w1"].clone())
        G, E, LP = make_models_be("sg2")
        b = LatentEmbedStep(G, E, LP, mode="W", generator="sg2", lr=0.005)
        b.begin_image(imgs1, w_init=w0)
        b.capture(imgs1, noises, warmup=1)
        b.begin_image(imgs1, w_init=w0)
        wb = [b.replay()["w1"].clone() for _ in range(5)]
        torch.cuda.synchronize()
        assert not torch.equal(wa[4], wa[0])
        for i in range(5):
            assert torch.equal(wa[i], wb[i]), (i, relerr(wb[i], wa[i].cpu().numpy()))
    finally:
        ops.set_deterministic(was)


def test_be_fullsize_sg2_1024_bf16_eager_and_replay():
    """StyleGAN2-1024 + E.BE(16, 512, 9) (18 W+ rows), bf16, batch 1, W mode: 2 eager iterations and 2 replayed ones from the same
    start and the same static noise; all finite, replay within the band test_fullsize_sg2_1024_bf16_eager_and_replay allows for
    E_Blur, and the image gradient comes out of the encoder backward's one-launch last stage."""
    from dge_amd import ops
    from dge_amd.embedding_v2 import LatentEmbedStep, build_models_v2
    from dge_amd.encoder import BE
    from dge_amd.enc_steps import draw_noises
    from tests.helpers import s2_shapes
    torch.manual_seed(0)
    img = torch.tanh(R.randn("embed_v2.full.img", (1, 3, 1024, 1024), 7, 0.8)).cuda()
    PG = R.fill_s2(s2_shapes(1024), seed=1)

    def make():
        G, E, LP = build_models_v2(2, 1024, 16, "bf16", device=DEV, seed=3, encoder="be")
        G.load_state_dict(PG)
        LP.load_state_dict(LR.seeded_params(0))
        assert isinstance(E, BE) and G.synthesis.num_layers == 18 and E.layer_count == 9 and E.maxf == 512
        return LatentEmbedStep(G, E, LP, mode="W", generator="sg2", lr=0.005)
    w0 = R.randn("embed_v2.full.w0", (1, 18, 512), 5)
    a = make()
    ops.noise_seed(11)
    noises = (None, None, draw_noises(a.E, 1, 1024, img.device))
    a.begin_image(img, w_init=w0)
    a.opt.graph_begin(2, img.device)
    log = []
    ops.KERNEL_LOG = log
    try:
        wa = []
        for _ in range(2):
            a.opt.graph_advance()
            r = a.step(img, noises)
            wa.append(r["w1"].clone())
    finally:
        ops.KERNEL_LOG = None
    torch.cuda.synchronize()
    assert all(torch.isfinite(w).all() for w in wa) and torch.isfinite(r["imgs2"]).all() and np.isfinite(float(r["loss_msiv"]))
    assert np.isfinite(float(r["loss_mslv"])) and all(p.grad is None for p in a.E.parameters())
    assert sum(n == "in_bwd_fromrgb_img<bf16,data>" for n, _ in log) == 2, sorted({n for n, _ in log})
    b = make()
    b.begin_image(img, w_init=w0)
    b.capture(img, noises, warmup=1)
    b.begin_image(img, w_init=w0)
    wb = [b.replay()["w1"].clone() for _ in range(2)]
    torch.cuda.synchronize()
    rb = b.last
    assert all(torch.isfinite(w).all() for w in wb) and np.isfinite(float(rb["loss_msiv"])) and np.isfinite(float(rb["loss_mslv"]))
    for i in range(2):
        e = l2rel(wb[i], wa[i].cpu().numpy())
        meas(f"embed_v2_be.full.W.it{i}", w1_l2=e)
        assert e < (2e-2 if i == 0 else 8e-2), (i, e)
