#!/usr/bin/env python3
"""Golden vectors for the differentiable StyleGAN2 mapping and the Z-space v2 inversion loop (dge_amd.embedding_v2, mode "Z") from
the reference's own modules.

Runs ONLY in the build container (needs the reference tree; a no-op elsewhere).  Imports the reference modules (never copies them)
through tools/gen_golden.py's stubs and helpers.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_s2_mapping.py [s2_mapping_grad] [embed_v2_z]

s2_mapping_grad.npz : the reference StyleGAN2Generator at 64^2 (fmaps_base 2048, fmaps_max 128: 10 W+ rows, the model of
                      s2_small.npz with tests/s2z_models.py's mapping weights), z [3, 512]: w; wp and d/dz of (wp * gw).sum() for (psi, layers) = (0.7, 8), (0.7, 10) and no
                      truncation; d/dz of (image * gi).sum() through the synthesis (eval mode, randomize_noise=False, psi 0.7 on 8
                      layers, the call of baseline_utils/image2stylegan_w2z_opW.py).
embed_v2_z.npz      : two iterations of the mode-Z loop of embedding_v2.py's docstring (the v2 loop with the latent in front of
                      the mapping network; the reference has no such script), composed from the reference's generators, E_Blur,
                      space_loss and LREQAdam: StyleGAN2 and StyleGAN1, B = 2, 64^2, the seeded LPIPS stand-in.
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG          # noqa: E402  (exits when the reference is absent; installs the torchvision / PIL stubs)

import numpy as np               # noqa: E402
import torch                     # noqa: E402

from tests.golden import recipe as R        # noqa: E402

shapes_of = GG.shapes_of
TRUNC_CASES = (("t8", 0.7, 8), ("t10", 0.7, 10), ("none", None, None))


def _s2_generator():
    from model.stylegan2_generator import StyleGAN2Generator
    from tests.s2z_models import S2Z_KW, s2z_state_dict
    G = StyleGAN2Generator(64, **S2Z_KW)
    G.load_state_dict(s2z_state_dict())          # (mapping weights at a real checkpoint's scale: w = O(1))
    G.eval()
    for p_ in G.parameters():
        p_.requires_grad_(False)
    return G


def gen_s2_mapping_grad():
    G = _s2_generator()

    def margin_of(z):          # smallest |pre-activation| of the mapping's leaky-relus, relative to the largest of its layer
        with GG._LreluTap() as tap, torch.no_grad():
            G.mapping(z)
        return min(float(x.abs().min()) / float(x.abs().max()) for x in tap.inputs)
    # 12288 pre-activations: a seeded z usually has one within 1e-5 of the kink; take the first seed whose z has none
    z_seed = next(sd for sd in range(81, 181) if margin_of(R.randn("s2map.z", (3, 512), sd)) > 2e-5)
    z0 = R.randn("s2map.z", (3, 512), z_seed)
    out = {"z": z0, "z_seed": np.array(z_seed), "w_avg": G.truncation.w_avg.clone()}
    margins = []
    for tag, psi, layers in TRUNC_CASES:
        z = z0.clone().requires_grad_(True)
        with GG._LreluTap() as tap:
            w = G.mapping(z)["w"]
        margins.append(min(float(x.abs().min()) / float(x.abs().max()) for x in tap.inputs))
        wp = G.truncation(w, psi, layers)
        gw = R.randn("s2map.gw." + tag, tuple(wp.shape), 82)
        (wp * gw).sum().backward()
        out["w"], out["wp_" + tag], out["dz_" + tag] = w.detach(), wp.detach(), z.grad.clone()
    assert min(margins) > 1e-5, margins          # no mapping pre-activation within rounding of the leaky-relu kink
    out["kink_margin"] = np.array(min(margins))
    z = z0.clone().requires_grad_(True)
    img = G(z, trunc_psi=0.7, trunc_layers=8, randomize_noise=False)["image"]
    gi = R.randn("s2map.gi", tuple(img.shape), 83)
    (img * gi).sum().backward()
    out["image_norm"], out["dz_image"] = img.detach().norm(), z.grad.clone()
    GG.save_npz("s2_mapping_grad.npz", **out)


ITERATIONS, LR, NORM_P, PSI = 2, 0.005, 2, 0.7


def gen_embed_v2_z():
    import model.stylegan1.net as SG1
    import model.E.E_Blur as EB
    import training_utils as TU
    from model.utils.custom_adam import LREQAdam
    from oracle import lpips_ref as LRF

    L, B = 5, 2
    LP = LRF.seeded_params(0)
    lp = lambda a, b: LRF.lpips(LP, a, b)
    imgs1 = torch.tanh(R.randn("embed_v2_z.img", (B, 3, 64, 64), 73, 0.8))
    out = {"imgs1": imgs1}
    flat = lambda inf: [inf[0][0], inf[0][1], inf[0][2], inf[1], inf[2], inf[3], inf[4]]
    for gen in ("sg2", "sg1"):
        if gen == "sg1":
            Gs = SG1.Generator(startf=16, maxf=64, layer_count=L, latent_size=512, channels=3)
            sd = R.fill_encoder(shapes_of(Gs.state_dict()), seed=43)
            for k in sd:
                if k.endswith("blur.weight"):
                    sd[k] = Gs.state_dict()[k].clone()
                if k == "const":
                    sd[k] = R.randn("sg1step.const", tuple(sd[k].shape), 43)
            Gs.load_state_dict(sd)
            Gm = SG1.Mapping(num_layers=2 * L, mapping_layers=8, latent_size=512, dlatent_size=512, mapping_fmaps=512)
            Gm.load_state_dict({k: R.randn("sg1step.m." + k, tuple(v.shape), 44, 0.05 if k.endswith("weight") else 0.01)
                                for k, v in Gm.state_dict().items()})
            Gm.buffer1 = R.randn("sg1step.buffer1", (2 * L, 512), 44, 0.5)
            layer_idx = torch.arange(2 * L)[np.newaxis, :, np.newaxis]
            ones = torch.ones(layer_idx.shape, dtype=torch.float32)
            coefs = torch.where(layer_idx < L, PSI * ones, ones)
            wp_of = lambda z: Gm(z, coefs_m=coefs)
            gfun = lambda wp: Gs.forward(wp, L - 1)
            beta = 1e-3
        else:
            G2 = _s2_generator()
            wp_of = lambda z: G2.truncation(G2.mapping(z)["w"], PSI, G2.num_layers)          # psi on every row
            gfun = lambda wp: G2.synthesis(wp, randomize_noise=False)["image"]
            beta = 3e-4
        E = EB.BE(startf=16, maxf=64, layer_count=L)
        esd = R.fill_encoder(shapes_of(E.state_dict()), seed=71)
        for k in esd:
            if k.endswith("blur.weight"):
                esd[k] = E.state_dict()[k].clone()
        E.load_state_dict(esd)
        for p_ in E.parameters():
            p_.requires_grad_(False)
        const2 = None
        if gen == "sg1":          # the const term of W mode: const2 = E(imgs1)'s const output, a constant
            with GG._NoiseFeeder(f"embed_v2_z.{gen}.init", 2) as nf:
                const2 = E(imgs1)[0].detach()
            out[f"{gen}_init_noise_shapes"] = np.array([list(s_) for s_ in nf.log])
        z = R.randn(f"embed_v2_z.{gen}.z0", (B, 512), 5).requires_grad_(True)
        out[f"{gen}_z0"] = z.detach().clone()
        opt = LREQAdam([{"params": z}], lr=LR, betas=(0.0, 0.99), weight_decay=0)
        for it in range(ITERATIONS):
            pre = f"{gen}_it{it}"
            with GG._NoiseFeeder(f"embed_v2_z.{gen}.it{it}", 2) as nf, warnings.catch_warnings():
                warnings.simplefilter("ignore")
                split = [nf.i]
                wp = wp_of(z)
                imgs2 = gfun(wp)
                split.append(nf.i)
                if gen == "sg1":
                    const3, w2 = E(imgs2)
                l_i, i_i = TU.space_loss(imgs1, imgs2, lpips_model=lp)
                m1 = imgs1[:, :, :, imgs1.shape[3] // 8:-imgs1.shape[3] // 8]
                m2 = imgs2[:, :, :, imgs2.shape[3] // 8:-imgs2.shape[3] // 8]
                l_m, i_m = TU.space_loss(m1, m2, lpips_model=lp)
                o = imgs1.shape[2] // 8 + imgs1.shape[2] // 32
                l_s, i_s = TU.space_loss(imgs1[:, :, o:-o, o:-o], imgs2[:, :, o:-o, o:-o], lpips_model=lp)
                loss_msiv = l_i + l_m * 0.125 * 3 + l_s * 0.125 * 5
                opt.zero_grad()
                loss_msiv.backward(retain_graph=True)
                out[f"{pre}_grad1"] = z.grad.clone()
                opt.step()
                out[f"{pre}_z_mid"] = z.detach().clone()
                if gen == "sg2":
                    const3, w2 = E(imgs2)
                split.append(nf.i)
                wp_new = wp_of(z)          # the direct term of phase 2 sees the updated code
                l_w, i_w = TU.space_loss(wp_new, w2, image_space=False)
                lat, l_c = l_w, torch.tensor(0.0)
                if const2 is not None:
                    l_c, _ = TU.space_loss(const2, const3, image_space=False)
                    lat = l_w + l_c
                norm = torch.norm(z, p=NORM_P)
                loss_mslv = lat * 0.01 + beta * norm
                opt.zero_grad()
                loss_mslv.backward()
                out[f"{pre}_grad2"] = z.grad.clone()
                opt.step()
            if it == 0:
                out[f"{gen}_noise_shapes"] = np.array([list(s_) for s_ in nf.log])
                out[f"{gen}_noise_split"] = np.array(split)
            out[f"{pre}_z"] = z.detach().clone()
            out[f"{pre}_wp"] = wp.detach().clone()
            out[f"{pre}_wp_new"] = wp_new.detach().clone()
            out[f"{pre}_w2"] = w2.detach().clone()
            out[f"{pre}_imgs2"] = imgs2.detach().clone()
            out[f"{pre}_losses"] = np.array([float(loss_msiv), float(l_i), float(l_m), float(l_s), float(l_w), float(l_c), float(norm),
                                             float(loss_mslv)])
            out[f"{pre}_info"] = np.array([flat(i_i), flat(i_m), flat(i_s), flat(i_w)])
            print(gen, "it", it, out[f"{pre}_losses"])
    GG.save_npz("embed_v2_z.npz", **out)


SECTIONS = {"s2_mapping_grad": gen_s2_mapping_grad, "embed_v2_z": gen_embed_v2_z}

if __name__ == "__main__":
    for s_ in sys.argv[1:] or list(SECTIONS):
        print("==", s_)
        SECTIONS[s_]()
