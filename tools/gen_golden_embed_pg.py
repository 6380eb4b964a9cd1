#!/usr/bin/env python3
"""Golden vectors for the PGGAN real-image inversion (dge_amd.embedding_v2_pggan) from the reference's own modules.

Runs ONLY in the build container (needs /root/reference; a no-op elsewhere).  Imports the reference modules (never copies them)
through tools/gen_golden.py's stubs and helpers.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_embed_pg.py [encpg_imggrad] [embed_v2_pg]

encpg_imggrad.npz : E_PG.BE (model / inputs / functional of encpg_grad.npz) with the input image requiring a gradient: g_img, the
                    loss, the head output and every parameter gradient.
embed_v2_pg.npz   : two iterations of the v2 inversion loop (embedding_v2_styleGAN1.py:54-168) applied to PGGAN + E_PG in the
                    evident-intent form of SURVEY Q5 (the reference has no PGGAN inversion script): w2 is the
                    live output of `new_final`, there is no const term.  PGGAN 64 (fmaps_base 1024, fmaps_max 64), E_PG 5 blocks,
                    batch 2, mode E and mode W.
"""
import contextlib
import io
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


def _encoder():
    """The E_PG.BE of encpg_small.npz / encpg_grad.npz / step_pg.npz."""
    import model.E.E_PG as EP
    E = EP.BE(startf=32, maxf=512, layer_count=5, pggan=True)
    sd = R.fill_encoder(shapes_of(E.state_dict()), seed=62)
    for k in sd:
        if "instance_norm_3.weight" in k:
            sd[k] = R.randn("pg." + k, tuple(sd[k].shape), 62, 0.2, 1.0)
    E.load_state_dict(sd)
    return E


def gen_encpg_imggrad():
    """gen_encpggrad with img.requires_grad_(True): what phase 2 of the inversion loop back-propagates through E(imgs2).  The
    leaky-relu kinks are cleared for every pre-activation, FromRGB's included (its bias is the first owner)."""
    E = _encoder()
    img = R.randn("ep.img", (2, 3, 64, 64), 62, 0.5).requires_grad_(True)
    feats = {}
    E.new_final.register_forward_hook(lambda m_, i, o: feats.__setitem__("head", o))

    def run():
        with GG._NoiseFeeder("ep", 62):
            E(img)
    owners, names = GG.enc_kink_owners(E, "has_second_conv")
    assert names[0] == "FromRGB.from_rgb.bias"
    nudged, margin = GG.clear_kinks([run], owners, names)
    run()
    z = feats["head"]
    loss = (z * R.randn("ep.gz", tuple(z.shape), 64)).sum()
    loss.backward()
    out = {"loss": loss.detach(), "z": z.detach(), "g_img": img.grad, "kink_margin": np.array(margin),
           **{"param:" + k: v for k, v in nudged.items()}}
    for k, p_ in E.named_parameters():
        if p_.grad is None:
            continue
        g = p_.grad
        out["norm:" + k] = g.norm()
        out["grad:" + k] = g if g.numel() <= 4096 else g.flatten()[:4096]          # (the norm pins the rest: keeps the file small)
    GG.save_npz("encpg_imggrad.npz", **out)


PNAMES = ("decode_block.0.conv_1.weight", "decode_block.2.conv_2.weight", "decode_block.1.conv_3.weight",
          "decode_block.1.instance_norm_3.weight", "decode_block.1.bias_1", "FromRGB.from_rgb.weight", "new_final.bias")
ITERATIONS = 2
LR = 0.005
BETA = 1e-3
NORM_P = 2


def gen_embed_v2_pg():
    from model.pggan.pggan_generator import PGGANGenerator
    import training_utils as TU
    from model.utils.custom_adam import LREQAdam
    from oracle import lpips_ref as LRF

    B = 2
    LP = LRF.seeded_params(0)
    lp = lambda a, b: LRF.lpips(LP, a, b)
    imgs1 = torch.tanh(R.randn("embed_v2_pg.img", (B, 3, 64, 64), 73, 0.8))
    out = {"imgs1": imgs1}
    flat = lambda inf: [inf[0][0], inf[0][1], inf[0][2], inf[1], inf[2], inf[3], inf[4]]
    for mode in ("E", "W"):
        G = PGGANGenerator(64, fmaps_base=1024, fmaps_max=64)
        G.load_state_dict({k: (R.randn("pgstep." + k, tuple(v.shape), 51, 0.2 if k.endswith("bias") else 1.0) if v.ndim else v.clone())
                           for k, v in G.state_dict().items()})
        E = _encoder()
        feats = {}
        E.new_final.register_forward_hook(lambda m_, i, o, feats=feats: feats.__setitem__("head", o))

        def encode(x):
            E(x)
            return feats["head"]
        if mode == "E":
            opt = LREQAdam([{"params": E.parameters()}], lr=LR, betas=(0.0, 0.99), weight_decay=0)
        else:
            with GG._NoiseFeeder("embed_v2_pg.W.init", 2) as nf:
                z = encode(imgs1).detach()
            out["W_init_noise_shapes"] = np.array([list(s_) for s_ in nf.log])
            z.requires_grad = True
            out["W_z0"] = z.detach().clone()
            opt = LREQAdam([{"params": z}], lr=LR, betas=(0.0, 0.99), weight_decay=0)
        for it in range(ITERATIONS):
            pre = f"{mode}_it{it}"
            with GG._NoiseFeeder(f"embed_v2_pg.{mode}.it{it}", 2) as nf, warnings.catch_warnings(), \
                    contextlib.redirect_stdout(io.StringIO()):
                warnings.simplefilter("ignore")
                split = []
                if mode == "E":
                    z = encode(imgs1)
                split.append(nf.i)
                imgs2 = G(z)["image"]
                w2 = encode(imgs2)
                split.append(nf.i)
                # phase 1: the three-window image loss (embedding_v2_styleGAN1.py:94-117)
                l_i, i_i = TU.space_loss(imgs1, imgs2, lpips_model=lp)
                m1 = imgs1[:, :, :, imgs1.shape[3] // 8:-imgs1.shape[3] // 8]
                m2 = imgs2[:, :, :, imgs2.shape[3] // 8:-imgs2.shape[3] // 8]
                l_m, i_m = TU.space_loss(m1, m2, lpips_model=lp)
                o = imgs1.shape[2] // 8 + imgs1.shape[2] // 32
                s1, s2 = imgs1[:, :, o:-o, o:-o], imgs2[:, :, o:-o, o:-o]
                l_s, i_s = TU.space_loss(s1, s2, lpips_model=lp)
                loss_msiv = l_i + l_m * 0.125 * 3 + l_s * 0.125 * 5
                opt.zero_grad()
                loss_msiv.backward(retain_graph=True)
                out[f"{pre}_grad1"] = (z.grad if mode == "W" else E.FromRGB.from_rgb.weight.grad).clone()
                opt.step()
                # phase 2: the latent loss and the norm penalty (:119-131)
                l_w, i_w = TU.space_loss(z, w2, image_space=False)
                norm = torch.norm(z, p=NORM_P)
                loss_mslv = l_w * 0.01 + BETA * norm
                opt.zero_grad()
                loss_mslv.backward()
                out[f"{pre}_grad2"] = (z.grad if mode == "W" else E.FromRGB.from_rgb.weight.grad).clone()
                opt.step()
            if it == 0:
                out[f"{mode}_noise_shapes"] = np.array([list(s_) for s_ in nf.log])
                out[f"{mode}_noise_split"] = np.array(split)
            out[f"{pre}_z"] = z.detach().clone()
            out[f"{pre}_w2"] = w2.detach().clone()
            out[f"{pre}_imgs2"] = imgs2.detach().clone()
            out[f"{pre}_losses"] = np.array([float(loss_msiv), float(l_i), float(l_m), float(l_s), float(l_w), float(norm), float(loss_mslv)])
            out[f"{pre}_info"] = np.array([flat(i_i), flat(i_m), flat(i_s), flat(i_w)])
            if mode == "E":
                sd = E.state_dict()
                out[f"{pre}_param_checksum"] = np.array(R.checksum({k: v for k, v in sd.items() if v.dtype.is_floating_point}))
                for k in PNAMES:                # (a slice and the norm where the tensor is large)
                    out[f"{pre}_after_phase2:{k}"] = sd[k].clone() if sd[k].numel() <= 4096 else sd[k].flatten()[:4096].clone()
                    out[f"{pre}_after_phase2_norm:{k}"] = sd[k].norm()
            else:
                out[f"{pre}_param_checksum"] = np.array(R.checksum({"z": z.detach()}))
            print(mode, "it", it, out[f"{pre}_losses"])
    GG.save_npz("embed_v2_pg.npz", **out)


SECTIONS = {"encpg_imggrad": gen_encpg_imggrad, "embed_v2_pg": gen_embed_v2_pg}

if __name__ == "__main__":
    for s_ in sys.argv[1:] or list(SECTIONS):
        print("==", s_)
        SECTIONS[s_]()
