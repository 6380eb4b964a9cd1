#!/usr/bin/env python3
"""Golden runs of the two Cat256 mis-align iterations from the reference's own modules, in the manner of gen_step_misalign in
tools/gen_golden_gradcam.py (whose stubs for cv2 / torchvision, noise feeder and recipes are used as they are):
two iterations of the loop body of ablation_utils/Cat256/E_mis_align_case_1.py:109-206 and E_mis_align_case_2.py:110-214
(mtype 2) at the reduced size of step_misalign.npz - StyleGAN2-64 with fmaps_base=2048, fmaps_max=128, the narrow VGG16 of
R.GRADCAM_CFG, the seeded LPIPS stand-in, B = 2.

Runs ONLY where the reference is present (a no-op elsewhere).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_misalign_cases.py

Writes tests/golden/step_misalign_case1.npz and step_misalign_case2.npz; running it twice gives the same bytes (the archive is
written with fixed member dates).  Two departures from step_misalign.npz's setup, both forced:
  * the encoder is BE(16, 128, 5), not BE(16, 64, 5): loss_c compares the generator's constant [B,128,4,4] with the encoder's
    const2, which has maxf channels - with maxf = 64 the script's MSELoss refuses the shapes;
  * a committed file stays below 1 MiB, so a sampled tensor is stored as its first 2048 elements (the parameter checksum covers the
    whole state_dict after EVERY optimizer call), the calls that leave the parameters as they are (case 2's calls 2 and 3) store the
    checksum alone, and the `legacy` variant - the same run with `zero_grad(set_to_none=False)`, torch < 2.0's behaviour - stores
    losses, checksums, w2 and the sampled tensors after the last call of each iteration, not the masks.
"""
import contextlib
import io
import os
import sys
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_gradcam as GG      # noqa: E402  (exits when the reference is absent; stubs cv2 / torchvision, imports metric.grad_cam)

import types                         # noqa: E402

import numpy as np                   # noqa: E402
import torch                         # noqa: E402
from torch import nn                 # noqa: E402

from oracle import gradcam_ref as GR     # noqa: E402
from tests.golden import recipe as R    # noqa: E402

SAMPLED = ("decode_block.0.conv_1.weight", "decode_block.2.conv_2.weight", "decode_block.4.inver_mod2.weight",
           "decode_block.1.bias_1", "FromRGB.from_rgb.weight")
CLIP = 2048
ENC = dict(startf=16, maxf=128, layer_count=5)


def save_npz(path, arrays):
    """np.savez without the clock: stored members in sorted order, every member dated 1980-01-01"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def run(case, legacy):
    from model.stylegan2_generator import StyleGAN2Generator
    import model.E.E as EE
    tv = sys.modules["torchvision"]
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.Compose = lambda x: None
    tv.transforms.ToTensor = lambda: None
    sys.modules["torchvision.transforms"] = tv.transforms
    import training_utils as TU
    from model.utils.custom_adam import LREQAdam
    from oracle import lpips_ref as LR

    shapes_of = lambda sd: {k: list(v.shape) for k, v in sd.items()}
    G = StyleGAN2Generator(64, fmaps_base=2048, fmaps_max=128)
    G.load_state_dict(R.fill_s2(shapes_of(G.state_dict()), seed=11))
    E = EE.BE(maxf=ENC["maxf"], startf=ENC["startf"], layer_count=ENC["layer_count"])
    E.load_state_dict(R.fill_encoder(shapes_of(E.state_dict()), seed=31))
    LP = LR.seeded_params(0)
    for k, v in LP.items():
        if k.startswith("lin"):
            v.requires_grad_(True)
    lp = lambda a, b: LR.lpips(LP, a, b)
    cfg = R.GRADCAM_CFG
    net = GR.VGG16Ref(cfg["widths"], cfg["fc"], cfg["classes"])
    net.load_state_dict(GR.seeded_state(shapes_of(net.state_dict()), cfg["seed"]))
    final_layer = [n for n, m in net.named_modules() if isinstance(m, nn.Conv2d)][-1]
    gcpp = GG.GradCamPlusPlus(net, final_layer)
    gbp = GG.GuidedBackPropagation(net)
    opt = LREQAdam([{"params": E.parameters()}], lr=0.0015, betas=(0.0, 0.99), weight_decay=0)
    zero_grad = (lambda: opt.zero_grad(set_to_none=False)) if legacy else (lambda: opt.zero_grad(set_to_none=True))
    B = 2
    const1 = G.synthesis.early_layer(torch.zeros(B)).detach().clone()           # :61-62
    new_z = R.randn("step.new_z", (B, 512), 1)
    orig_randn_like = torch.randn_like
    torch.randn_like = lambda t, **kw: new_z.clone()
    flat = lambda inf: [inf[0][0], inf[0][1], inf[0][2], inf[1], inf[2], inf[3], inf[4]]
    out = {}

    def after(it, call, tensors):
        out[f"it{it}_call{call}_checksum"] = np.array(R.checksum(E.state_dict()))
        if tensors:
            for k in SAMPLED:
                out[f"it{it}_call{call}:{k}"] = E.state_dict()[k].detach().reshape(-1)[:CLIP].clone()

    try:
        for it in range(2):
            np.random.seed(it)
            z = R.randn(f"step.z{it}", (B, 512), 1)
            with torch.no_grad():
                r = G(z, trunc_psi=0.7, trunc_layers=8, randomize_noise=False)
            imgs1, w1 = r["image"], r["wp"]
            with GG._NoiseFeeder(f"step.it{it}", 1):
                const2, w2 = E(imgs1)
            imgs2 = G.synthesis(w2)["image"]
            zero_grad()
            with contextlib.redirect_stdout(io.StringIO()):
                mask_1 = gcpp(imgs1, None)
                mask_2 = gcpp(imgs2, None)
                imgs1_ = imgs1.detach().clone()
                imgs1_.requires_grad = True
                imgs2_ = imgs2.detach().clone()
                imgs2_.requires_grad = True
                grad_1 = gbp(imgs1_)
                grad_2 = gbp(imgs2_)
            heat_1, cam_1 = GG.mask2cam(mask_1, imgs1)
            heat_2, cam_2 = GG.mask2cam(mask_2, imgs2)
            l_grad, i_grad = TU.space_loss(grad_1, grad_2, lpips_model=lp)
            if case == 1:                                                   # E_mis_align_case_1.py:172-205
                l_imgs, i_imgs = TU.space_loss(imgs1.detach().clone(), imgs2.detach().clone(), lpips_model=lp)
                m1, m2 = mask_1.float(), mask_2.float()
                l_mask, i_mask = TU.space_loss(m1.detach().clone(), m2.detach().clone(), lpips_model=lp)
                c1, c2 = cam_1.float(), cam_2.float()
                l_cam, i_cam = TU.space_loss(c1.detach().clone(), c2.detach().clone(), lpips_model=lp)
                loss_tsa = l_imgs + l_mask + l_cam
                zero_grad()
                loss_tsa.backward(retain_graph=True)
                opt.step()
                after(it, 1, False)
                l_c, i_c = TU.space_loss(const1, const2, image_space=False)
                l_w, i_w = TU.space_loss(w1, w2, image_space=False)
                loss_mtv = (l_c + l_w) * 0.01
                zero_grad()
                loss_mtv.backward()
                opt.step()
                after(it, 2, True)
            else:                                                           # E_mis_align_case_2.py:172-214
                l_imgs, i_imgs = TU.space_loss(imgs1, imgs2, lpips_model=lp)
                zero_grad()
                l_imgs.backward(retain_graph=True)
                opt.step()
                after(it, 1, not legacy)
                m1 = mask_1.float()
                m1.requires_grad = True
                m2 = mask_2.float()
                m2.requires_grad = True
                l_mask, i_mask = TU.space_loss(m1, m2, lpips_model=lp)
                loss_mask = l_mask * 5.0
                zero_grad()
                loss_mask.backward(retain_graph=True)
                opt.step()
                after(it, 2, False)
                c1 = cam_1.float()
                c1.requires_grad = True
                c2 = cam_2.float()
                c2.requires_grad = True
                l_cam, i_cam = TU.space_loss(c1, c2, lpips_model=lp)
                loss_cam = l_cam * 9.0
                zero_grad()
                loss_cam.backward(retain_graph=True)
                opt.step()
                after(it, 3, False)
                l_c, i_c = TU.space_loss(const1, const2, image_space=False)
                l_w, i_w = TU.space_loss(w1, w2, image_space=False)
                zero_grad()
                l_w.backward()
                opt.step()
                after(it, 4, True)
            out[f"it{it}_w2"] = w2.detach()
            if not legacy:
                out[f"it{it}_mask_1"] = m1.detach()
                out[f"it{it}_mask_2"] = m2.detach()
            # the unweighted values; case 2 steps on imgs, 5 * mask, 9 * Gcam and w, case 1 on (c + w) * 0.01
            out[f"it{it}_losses"] = np.array([float(l_imgs), float(l_mask), float(l_cam), float(l_grad), float(l_w), float(l_c)])
            out[f"it{it}_info"] = np.array([flat(i_imgs), flat(i_mask), flat(i_cam), flat(i_grad), flat(i_w), flat(i_c)])
            print("case", case, "legacy" if legacy else "default", "it", it, out[f"it{it}_losses"])
    finally:
        torch.randn_like = orig_randn_like
    pre = "legacy_" if legacy else ""
    return {pre + k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def main():
    import warnings
    warnings.filterwarnings("ignore")
    for case in (1, 2):
        arrays = {"encoder": np.array([ENC["startf"], ENC["maxf"], ENC["layer_count"]]), "clip": np.array(CLIP)}
        arrays.update(run(case, legacy=False))
        arrays.update(run(case, legacy=True))
        path = os.path.join(GG.OUT, "step_misalign_case%d.npz" % case)
        save_npz(path, arrays)
        print("wrote", os.path.basename(path), os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
