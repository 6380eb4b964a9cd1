#!/usr/bin/env python3
"""Golden vectors for the BigGAN-deep real-image inversion (dge_amd.embedding_v2_biggan) from the reference's own modules.

Runs ONLY in the build container (needs /root/reference; a no-op elsewhere).  Imports the reference modules (never copies them)
through tools/gen_golden.py's stubs and helpers; the attention case adds the `cv2` stand-ins and the narrow vgg16-layout network of
tools/gen_golden_gradcam.py.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_embed_big.py [encbig_imggrad] [embed_v2_big]

encbig_imggrad.npz : E_BIG.BE (model / inputs of encbig_small.npz, train mode) with the input image requiring a gradient:
                     g_img, the loss and every parameter gradient of gen_encbiggrad's seeded functional.
embed_v2_big.npz   : two iterations of embedding_v2_BigGAN.py:78-165 at BIGGAN_SMALL_CFG (64x64), batch 2, for mode E, mode W and
                     mode W with the attention terms.
"""
import contextlib
import io
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG          # noqa: E402  (exits when the reference is absent; installs the torchvision / PIL stubs)

import numpy as np               # noqa: E402
import torch                     # noqa: E402
from torch import nn             # noqa: E402

from tests.golden import recipe as R        # noqa: E402

shapes_of = GG.shapes_of


def gen_encbig_imggrad():
    """gen_encbiggrad with img.requires_grad_(True): what embedding_v2_BigGAN.py:94,164 back-propagates through E(imgs2).  The
    leaky-relu kinks are cleared for every pre-activation, FromRGB's included (its bias is the first owner)."""
    import model.E.E_BIG as EBG
    E = EBG.BE(startf=32, maxf=512, layer_count=5, biggan=True)
    E.load_state_dict(R.fill_encbig(shapes_of(E.state_dict()), seed=81))
    E.train()
    img = R.randn("ebg.img", (2, 3, 64, 64), 81, 0.5).requires_grad_(True)
    cond = R.randn("ebg.cond", (2, 256), 81, 0.5)
    uv = {k: v.clone() for k, v in E.state_dict().items() if k.endswith(("weight_u", "weight_v"))}

    def run():
        with torch.no_grad():
            for k, v in E.state_dict().items():
                if k in uv:
                    v.copy_(uv[k])
        with GG._NoiseFeeder("ebg", 81):
            return E(img, cond)
    owners, names = GG.enc_kink_owners(E, "has_second_conv", third=True)
    assert names[0] == "FromRGB.from_rgb.bias"
    nudged, margin = GG.clear_kinks([run], owners, names)
    c_v, z = run()
    loss = (z * R.randn("ebg.gz", tuple(z.shape), 82)).sum() + (c_v * R.randn("ebg.gcv", tuple(c_v.shape), 82)).sum()
    loss.backward()
    out = {"loss": loss.detach(), "c_v": c_v.detach(), "z": z.detach(), "g_img": img.grad,
           "kink_margin": np.array(margin), **{"param:" + k: v for k, v in nudged.items()}}
    for k, p_ in E.named_parameters():
        if p_.grad is None:
            continue
        g = p_.grad
        out["norm:" + k] = g.norm()
        out["grad:" + k] = g if g.numel() <= 4096 else g.flatten()[:4096]          # (the norm pins the rest: keeps the file small)
    GG.save_npz("encbig_imggrad.npz", **out)


PNAMES = ("decode_block.0.conv_1.weight", "decode_block.2.conv_2.weight", "decode_block.1.conv_3.weight",
          "decode_block.1.batch_norm_1.scale.weight_orig", "decode_block.0.batch_norm_3.offset.weight_orig",
          "decode_block.1.batch_norm_2.scale.weight_u", "decode_block.1.bias_1", "FromRGB.from_rgb.weight", "new_final_2.bias")
ITERATIONS = 2
LABEL = 30
LR = 0.0003


def _attention():
    """Grad-CAM++ on the narrow vgg16-layout stand-in with the cv2 restatements, wired as embedding_v2_BigGAN.py:51-57 (Grad-CAM++
    and guided back-propagation share ONE network: the guided ReLU hooks act on every later backward)."""
    from oracle import gradcam_ref as GR
    cv2 = types.ModuleType("cv2")
    cv2.resize = lambda src, dsize: GR.cv2_resize_linear(src, dsize)
    cv2.applyColorMap = GR.cv2_apply_colormap
    cv2.COLORMAP_JET = GR.COLORMAP_JET
    sys.modules["cv2"] = cv2
    from metric.grad_cam import GradCamPlusPlus, GuidedBackPropagation, mask2cam
    cfg = R.GRADCAM_CFG
    net = GR.VGG16Ref(cfg["widths"], cfg["fc"], cfg["classes"])
    net.load_state_dict(GR.seeded_state(shapes_of(net.state_dict()), cfg["seed"]))
    final_layer = [n for n, m in net.named_modules() if isinstance(m, nn.Conv2d)][-1]
    gcpp = GradCamPlusPlus(net, final_layer)
    GuidedBackPropagation(net)
    return gcpp, mask2cam


def gen_embed_v2_big():
    GG._stub("boto3"); GG._stub("botocore"); GG._stub("botocore.exceptions", ClientError=Exception)
    GG._stub("requests")
    from model.biggan_generator import BigGAN
    from model.utils.biggan_config import BigGANConfig
    import model.E.E_BIG as EBG
    import training_utils as TU
    from model.utils.custom_adam import LREQAdam
    from oracle import lpips_ref as LRF

    B = 2
    LP = LRF.seeded_params(0)
    lp = lambda a, b: LRF.lpips(LP, a, b)
    imgs1 = torch.tanh(R.randn("embed_v2_big.img", (B, 3, 64, 64), 73, 0.8))
    out = {"imgs1": imgs1}
    flat = lambda inf: [inf[0][0], inf[0][1], inf[0][2], inf[1], inf[2], inf[3], inf[4]]
    for tag, mode, att in (("E", "E", False), ("W", "W", False), ("W-att", "W", True)):
        G = BigGAN(BigGANConfig.from_dict(GG.BIGGAN_SMALL_CFG))
        G.load_state_dict(R.fill_biggan(shapes_of(G.state_dict()), seed=71))
        E = EBG.BE(startf=32, maxf=512, layer_count=5, biggan=True)
        E.load_state_dict(R.fill_encbig(shapes_of(E.state_dict()), seed=81))
        gcpp, mask2cam = _attention() if att else (None, None)
        # :37-47
        label = TU.one_hot((np.array(LABEL) * np.ones(B)).astype(np.int64))
        conditions = torch.tensor(label, dtype=torch.float)
        truncation = torch.tensor(0.4, dtype=torch.float)
        embed = G.embeddings(conditions)
        z0 = torch.tensor(TU.truncated_noise_sample(truncation=0.4, batch_size=B, seed=ITERATIONS % 30000), dtype=torch.float)
        cond_vector = torch.cat((z0, embed), dim=1)
        out[f"{tag}_cond_vector"] = cond_vector.detach().clone()
        if mode == "E":
            opt = LREQAdam([{"params": E.parameters()}], lr=LR, betas=(0.0, 0.99), weight_decay=0.0)
        else:
            with GG._NoiseFeeder(f"embed_v2_big.{tag}.init", 2) as nf:
                const1, w1_ = E(imgs1, cond_vector)
            out[f"{tag}_init_noise_shapes"] = np.array([list(s_) for s_ in nf.log])
            w1 = w1_.detach()
            w1.requires_grad = True
            out[f"{tag}_w0"] = w1.detach().clone()
            out[f"{tag}_const1"] = const1.detach().clone()
            opt = LREQAdam([{"params": w1}], lr=LR, betas=(0.0, 0.99), weight_decay=0)
        for it in range(ITERATIONS):
            pre = f"{tag}_it{it}"
            with GG._NoiseFeeder(f"embed_v2_big.{tag}.it{it}", 2) as nf, warnings.catch_warnings():
                warnings.simplefilter("ignore")
                split = []
                if mode == "E":
                    const1, w1 = E(imgs1, cond_vector)
                split.append(nf.i)
                imgs2, _ = G(w1, conditions, truncation)
                const2, w2 = E(imgs2, cond_vector)
                split.append(nf.i)
                loss_imgs, i_imgs = TU.space_loss(imgs1, imgs2, lpips_model=lp)
                loss_msiv = loss_imgs
                rows = [flat(i_imgs)]
                if att:
                    with contextlib.redirect_stdout(io.StringIO()):
                        mask_1 = gcpp(imgs1, None)
                        mask_2 = gcpp(imgs2, None)
                    _, cam_1 = mask2cam(mask_1, imgs1)
                    _, cam_2 = mask2cam(mask_2, imgs2)
                    mask_1, mask_2, cam_1, cam_2 = mask_1.float(), mask_2.float(), cam_1.float(), cam_2.float()
                    loss_mask, i_mask = TU.space_loss(mask_1.detach().clone(), mask_2.detach().clone(), lpips_model=lp)
                    loss_cam, i_cam = TU.space_loss(cam_1.detach().clone(), cam_2.detach().clone(), lpips_model=lp)
                    loss_msiv = loss_imgs + loss_mask + loss_cam
                    rows += [flat(i_mask), flat(i_cam)]
                    out[f"{pre}_mask_2"] = mask_2
                    out[f"{pre}_att_losses"] = np.array([float(loss_mask), float(loss_cam)])
                opt.zero_grad()
                loss_msiv.backward(retain_graph=True)
                if mode == "W":
                    out[f"{pre}_grad1:w1"] = w1.grad.clone()
                else:
                    out[f"{pre}_grad1:FromRGB.from_rgb.weight"] = E.FromRGB.from_rgb.weight.grad.clone()
                opt.step()
                loss_w, i_w = TU.space_loss(w1, w2, image_space=False)
                loss_c2, i_c2 = TU.space_loss(const1, const2, image_space=False)
                loss_mslv = loss_w * 0.01
                opt.zero_grad()
                loss_mslv.backward(retain_graph=True)
                if mode == "W":
                    out[f"{pre}_grad2:w1"] = w1.grad.clone()
                else:
                    out[f"{pre}_grad2:FromRGB.from_rgb.weight"] = E.FromRGB.from_rgb.weight.grad.clone()
                opt.step()
            if it == 0:
                out[f"{tag}_noise_shapes"] = np.array([list(s_) for s_ in nf.log])
                out[f"{tag}_noise_split"] = np.array(split)
            out[f"{pre}_w1"] = w1.detach().clone()
            out[f"{pre}_w2"] = w2.detach().clone()
            out[f"{pre}_imgs2"] = imgs2.detach()[:, :, ::2, ::2].clone()        # every second pixel: keeps the file small
            out[f"{pre}_imgs2_norm"] = imgs2.detach().norm()
            if mode == "E":
                out[f"{pre}_const1"] = const1.detach().clone()
            out[f"{pre}_const2"] = const2.detach().clone()
            out[f"{pre}_losses"] = np.array([float(loss_msiv), float(loss_imgs), float(loss_w), float(loss_c2), float(loss_mslv)])
            out[f"{pre}_info"] = np.array(rows + [flat(i_w), flat(i_c2)])
            if mode == "E":
                sd = E.state_dict()
                out[f"{pre}_param_checksum"] = np.array(R.checksum({k: v for k, v in sd.items() if v.dtype.is_floating_point}))
                for k in PNAMES:                # (a slice and the norm where the tensor is large)
                    out[f"{pre}_after_phase2:{k}"] = sd[k].clone() if sd[k].numel() <= 4096 else sd[k].flatten()[:4096].clone()
                    out[f"{pre}_after_phase2_norm:{k}"] = sd[k].norm()
            else:
                out[f"{pre}_param_checksum"] = np.array(R.checksum({"w1": w1.detach()}))
            print(tag, "it", it, out[f"{pre}_losses"])
    GG.save_npz("embed_v2_big.npz", **out)


SECTIONS = {"encbig_imggrad": gen_encbig_imggrad, "embed_v2_big": gen_embed_v2_big}

if __name__ == "__main__":
    for s_ in sys.argv[1:] or list(SECTIONS):
        print("==", s_)
        SECTIONS[s_]()
