#!/usr/bin/env python3
"""Golden vectors for the noise-map optimisation of the StyleGAN2 inversion (dge_amd.embedding_v2, optimize_noise) from the
reference's own modules.

Runs ONLY in the build container (needs the reference tree; a no-op elsewhere).  Imports the reference modules (never copies them)
through tools/gen_golden.py's stubs and helpers; writes under tests/golden/ only.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_s2_noise.py [s2_noise_grad] [embed_v2_noise]

s2_noise_grad.npz   : the reference StyleGAN2Generator at 64^2 (tests/s2_noise_models.py: the model of s2_small.npz with every
                      noise strength at magnitude about 0.1), wp [2, 10, 512]: the image and d<image, gimg>/d noise buffer of every
                      conv layer with the buffers as leaves (shared maps: the reference as it is), and the same with a map per row
                      (the reference run one row at a time on that row's maps); `param:` entries: the conv biases moved off the
                      leaky-relu kink for these three forwards (GG.clear_kinks), `kink_margin` the distance reached.  Plus the regulariser of StyleGAN2's projector -
                      written here with avg_pool2d / torch.roll and float64 autograd, not taken from the reference tree - on
                      seeded maps of side 4, 8, 16, 64 (three rows): values and gradients.
embed_v2_noise.npz  : two iterations of the mode-W StyleGAN2 loop of embedding_v2.py's docstring with the noise buffers optimised
                      beside w1, composed from the reference's generator, E_Blur, space_loss and LREQAdam: B = 2, 64^2, f32, the
                      seeded LPIPS stand-in; phase 1 back-propagates loss_msiv + 1e5 * sum reg, the maps take one LREQAdam step
                      of their own and are renormalised.
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG          # noqa: E402  (exits when the reference is absent; installs the torchvision / PIL stubs)

import numpy as np               # noqa: E402
import torch                     # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tests.golden import recipe as R        # noqa: E402
from tests.s2_noise_models import S2N_KW, S2N_RES, s2n_state_dict        # noqa: E402

shapes_of = GG.shapes_of
REG_SIDES = (4, 8, 16, 64)


def projector_reg(n):
    """StyleGAN2's projector (projector.py: the noise regularisation loop) on one map n [1, 1, R, R]."""
    total = 0.0
    while True:
        total = total + (n * torch.roll(n, shifts=1, dims=3)).mean() ** 2 + (n * torch.roll(n, shifts=1, dims=2)).mean() ** 2
        if n.shape[2] <= 8:
            return total
        n = F.avg_pool2d(n, kernel_size=2)


def _generator():
    from model.stylegan2_generator import StyleGAN2Generator
    G = StyleGAN2Generator(64, **S2N_KW)
    G.load_state_dict(s2n_state_dict())
    G.eval()
    for p_ in G.parameters():
        p_.requires_grad_(False)
    return G


def _layers(G):
    return [getattr(G.synthesis, f"layer{i}") for i in range(len(S2N_RES))]


def _set_noise(G, maps):
    """The noise buffers of the conv layers replaced by leaves [1, 1, R, R]."""
    for L, m in zip(_layers(G), maps):
        L._buffers["noise"] = m.reshape(1, 1, *m.shape[-2:]).clone().requires_grad_(True)
    return [L.noise for L in _layers(G)]


def gen_s2_noise_grad():
    G = _generator()
    wp = R.randn("s2n.wp", (2, 10, 512), 5)
    row_maps = lambda b: [R.randn(f"s2n.noise{i}", (2, r, r), 7)[b] for i, r in enumerate(S2N_RES)]
    buffers = [L.noise.detach().clone() for L in _layers(G)]

    # the three forwards of this fixture share the conv layers' biases: each is moved by the smallest amount that keeps every
    # leaky-relu pre-activation of all three away from the kink (GG.clear_kinks: the slope of an element within rounding of 0 is
    # decided by the last bit of whoever computes it, and one flipped element moves a whole pixel of g_noise)
    def forward(maps, w):
        _set_noise(G, maps)
        G.synthesis(w, randomize_noise=False)
    runs = [lambda: forward(buffers, wp)] + [lambda b=b: forward(row_maps(b), wp[b:b + 1]) for b in range(2)]
    nudged, margin = GG.clear_kinks(runs, [L.bias for L in _layers(G)], [f"synthesis.layer{i}.bias" for i in range(len(S2N_RES))])
    out = {"param:" + k: v for k, v in nudged.items()}
    out["kink_margin"] = np.array(margin)
    _set_noise(G, buffers)
    leaves = _set_noise(G, [L.noise.detach() for L in _layers(G)])
    img = G.synthesis(wp, randomize_noise=False)["image"]
    gimg = R.randn("s2n.gimg", tuple(img.shape), 5, 1.0 / img.numel() ** 0.5)
    (img * gimg).sum().backward()
    out["image_shared"] = img.detach()
    for i, n in enumerate(leaves):
        out[f"g_shared{i}"] = n.grad.reshape(1, *n.shape[-2:]).clone()
    imgs, grads = [], [[] for _ in S2N_RES]
    for b in range(2):
        leaves = _set_noise(G, row_maps(b))
        img = G.synthesis(wp[b:b + 1], randomize_noise=False)["image"]
        (img * gimg[b:b + 1]).sum().backward()
        imgs.append(img.detach())
        for i, n in enumerate(leaves):
            grads[i].append(n.grad.reshape(1, *n.shape[-2:]).clone())
    out["image_rows"] = torch.cat(imgs)
    for i, gl in enumerate(grads):
        out[f"g_rows{i}"] = torch.cat(gl)
    for r in REG_SIDES:
        n = R.randn(f"s2n.reg{r}", (3, r, r), 9, 1.3, 0.2).double().requires_grad_(True)
        vals = torch.stack([projector_reg(n[b].reshape(1, 1, r, r)) for b in range(3)])
        vals.sum().backward()
        out[f"reg{r}"], out[f"reg_grad{r}"] = vals.detach(), n.grad.clone()
    GG.save_npz("s2_noise_grad.npz", **out)


ITERATIONS, LR, NOISE_REG = 2, 0.005, 1e5


def gen_embed_v2_noise():
    import model.E.E_Blur as EB
    import training_utils as TU
    from model.utils.custom_adam import LREQAdam
    from oracle import lpips_ref as LRF

    L, B = 5, 2
    LP = LRF.seeded_params(0)
    lp = lambda a, b: LRF.lpips(LP, a, b)
    imgs1 = torch.tanh(R.randn("embed_v2_z.img", (B, 3, 64, 64), 73, 0.8))          # (the images of embed_v2_z.npz)
    out = {"imgs1": imgs1}
    G2 = _generator()
    avg = G2.truncation.w_avg
    gfun = lambda w: G2.synthesis(avg + 0.7 * (w - avg), randomize_noise=False)["image"]
    beta = 3e-4
    E = EB.BE(startf=16, maxf=64, layer_count=L)
    esd = R.fill_encoder(shapes_of(E.state_dict()), seed=71)
    for k in esd:
        if k.endswith("blur.weight"):
            esd[k] = E.state_dict()[k].clone()
    E.load_state_dict(esd)
    for p_ in E.parameters():
        p_.requires_grad_(False)
    w1 = R.randn("embed_v2_noise.w0", (B, 2 * L, 512), 5).requires_grad_(True)
    out["w0"] = w1.detach().clone()
    maps = _set_noise(G2, [L_.noise.detach() for L_ in _layers(G2)])
    opt = LREQAdam([{"params": w1}], lr=LR, betas=(0.0, 0.99), weight_decay=0)
    nopt = LREQAdam([{"params": maps}], lr=LR, betas=(0.0, 0.99), weight_decay=0)
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).clone()
    for it in range(ITERATIONS):
        pre = f"it{it}"
        with GG._NoiseFeeder(f"embed_v2_noise.it{it}", 2) as nf, warnings.catch_warnings():
            warnings.simplefilter("ignore")
            split = [nf.i]
            imgs2 = gfun(w1)
            split.append(nf.i)
            l_i, _ = TU.space_loss(imgs1, imgs2, lpips_model=lp)
            m1 = imgs1[:, :, :, imgs1.shape[3] // 8:-imgs1.shape[3] // 8]
            m2 = imgs2[:, :, :, imgs2.shape[3] // 8:-imgs2.shape[3] // 8]
            l_m, _ = TU.space_loss(m1, m2, lpips_model=lp)
            o = imgs1.shape[2] // 8 + imgs1.shape[2] // 32
            l_s, _ = TU.space_loss(imgs1[:, :, o:-o, o:-o], imgs2[:, :, o:-o, o:-o], lpips_model=lp)
            loss_msiv = l_i + l_m * 0.125 * 3 + l_s * 0.125 * 5
            reg = sum(projector_reg(n) for n in maps)
            opt.zero_grad()
            nopt.zero_grad()
            (loss_msiv + NOISE_REG * reg).backward(retain_graph=True)
            out[f"{pre}_grad1"] = w1.grad.clone()
            out[f"{pre}_noise_grad"] = cat([n.grad for n in maps])
            opt.step()
            nopt.step()
            with torch.no_grad():
                for n in maps:
                    n -= n.mean()
                    n *= n.square().mean().rsqrt()
            const3, w2 = E(imgs2)
            split.append(nf.i)
            l_w, _ = TU.space_loss(w1, w2, image_space=False)
            nrm = w1.norm(p=2)
            loss_mslv = l_w * 0.01 + nrm * beta
            opt.zero_grad()
            loss_mslv.backward()
            out[f"{pre}_grad2"] = w1.grad.clone()
            opt.step()          # (phase 2 reaches the maps through E(imgs2); no optimiser reads that gradient: the maps step once, in phase 1)
        if it == 0:
            out["noise_shapes"] = np.array([list(s_) for s_ in nf.log])
            out["noise_split"] = np.array(split)
        out[f"{pre}_w1"] = w1.detach().clone()
        out[f"{pre}_w2"] = w2.detach().clone()
        out[f"{pre}_imgs2"] = imgs2.detach().clone()
        out[f"{pre}_noise"] = cat(maps)
        out[f"{pre}_losses"] = np.array([float(loss_msiv), float(l_i), float(l_m), float(l_s), float(l_w), 0.0, float(nrm), float(loss_mslv)])
        out[f"{pre}_reg"] = np.array(float(reg))
        print("it", it, out[f"{pre}_losses"], float(reg))
    GG.save_npz("embed_v2_noise.npz", **out)


SECTIONS = {"s2_noise_grad": gen_s2_noise_grad, "embed_v2_noise": gen_embed_v2_noise}

if __name__ == "__main__":
    for s_ in sys.argv[1:] or list(SECTIONS):
        print("==", s_)
        SECTIONS[s_]()
