#!/usr/bin/env python3
"""Golden vectors for the independent-rows form of the BigGAN-deep inversion (embedding_v2_biggan.BigEmbedRowsStep) and its per-row
attention pieces, from the reference's own modules.

Runs ONLY in the build container (needs the reference checkout; a no-op elsewhere).  Imports the reference modules (never copies them)
through the stubs and helpers of tools/gen_golden.py and tools/gen_golden_embed_big.py.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_embed_big_rows.py [gradcam_rows] [embed_v2_big_rows]

gradcam_rows.npz      : GRADCAM_CFG's network and input size, N = 3: GradCamPlusPlus.call_per_image(imgs, None) (grad_cam.py:122-155)
                        and mask2cam on every one-row slice.  The images are searched (recipe tag + per-row scale, both stored) until
                        (a) the rows' arg-max classes are not all equal, (b) the coupled __call__ mask of some row differs from its
                        per-image mask by more than 10x the mask tolerance of tests/test_gradcam.py, (c) the coupled mask2cam of some
                        row differs from its one-row result by 10x the cam tolerance (the rows are scaled up towards the last one,
                        so a later row holds the batch's minimum).
embed_v2_big_rows.npz : three images at BIGGAN_SMALL_CFG (64x64) with the labels 30, 207, 5, mode W without and with the attention
                        terms, two iterations: every image run by the loop of embedding_v2_BigGAN.py:78-165 at batch 1 with its own
                        label, every run from the same (freshly loaded) weight_u / weight_v buffers and the same noise feed.  The keys
                        of embed_v2_big.npz, stacked per row.  The images are scaled by 1, 0.7 and 0.45, so that the rows' losses
                        lie apart and a coupled batch cannot pass for a row.
"""
import contextlib
import io
import os
import sys
import warnings

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG                  # noqa: E402  (exits when the reference is absent; installs the torchvision / PIL stubs)
import gen_golden_embed_big as GB        # noqa: E402

import numpy as np               # noqa: E402
import torch                     # noqa: E402

from tests.golden import recipe as R        # noqa: E402

MASK_TOL, CAM_TOL = 2e-3, 1e-2           # tests/test_gradcam.py: mask and cam bounds of the coupled forms against gradcam.npz
SCALES = (0.3, 0.65, 1.0)
LABELS = (30, 207, 5)
IMG_SCALES = (1.0, 0.7, 0.45)
ITERATIONS = GB.ITERATIONS
LR = GB.LR


def gen_gradcam_rows():
    cfg = R.GRADCAM_CFG
    N, H, W = 3, cfg["H"], cfg["W"]
    gcpp, mask2cam = GB._attention()
    scale = torch.tensor(SCALES).view(N, 1, 1, 1)
    for seed in range(200):
        tag = f"rows{seed}"
        imgs = R.gradcam_images(tag, N, H, W) * scale
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            logits = gcpp.net(imgs).detach().numpy()
            index = logits.argmax(1)
            srt = np.sort(logits, axis=1)
            margin = (srt[:, -1] - srt[:, -2]) / np.abs(logits).max()
            if len(set(index.tolist())) == 1 or margin.min() < 1e-2:          # (a), with arg-maxima a float32 path cannot reorder
                continue
            rows = np.asarray(gcpp.call_per_image(imgs, None), dtype=np.float64).copy()          # [N,H,W]
            coupled = gcpp(imgs, None).numpy()[:, 0]
            singles = np.stack([gcpp(imgs[b:b + 1], None).numpy()[0, 0] for b in range(N)])
        d_mask = np.abs(coupled - rows).reshape(N, -1).max(1)
        if d_mask.max() <= 10 * MASK_TOL:                                     # (b)
            continue
        # the per-image mask of the batch is the coupled call on the one-row slice
        assert np.abs(singles - rows).max() < 1e-5, np.abs(singles - rows).max()
        mask_t = torch.tensor(rows).view(N, 1, H, W)
        heat_c, cam_c = mask2cam(mask_t, imgs)
        one = [mask2cam(mask_t[b:b + 1], imgs[b:b + 1]) for b in range(N)]
        heat = torch.cat([h for h, _ in one]).numpy()
        cam = torch.cat([c for _, c in one]).numpy()
        d_cam = np.abs(cam_c.numpy() - cam).reshape(N, -1).max(1)
        if d_cam.max() <= 10 * CAM_TOL:                                       # (c)
            continue
        assert float(imgs[1:].min()) < float((torch.tensor(heat[0]) + imgs[0]).min())      # a later row holds the batch's minimum
        print("gradcam_rows: tag", tag, "index", index, "margin", margin, "d_mask", d_mask, "d_cam", d_cam)
        GG.save_npz("gradcam_rows.npz", img_tag=np.array(tag), img_scale=np.array(SCALES, dtype=np.float32), index=index.astype(np.int32),
                    logits=logits, margin=margin, mask_rows=rows.astype(np.float32).reshape(N, 1, H, W), heat_rows=heat, cam_rows=cam,
                    mask_coupled_diff=d_mask, cam_coupled_diff=d_cam, mask_diff_row=np.array(int(d_mask.argmax())),
                    cam_diff_row=np.array(int(d_cam.argmax())))
        return
    raise SystemExit("gradcam_rows: no image set met (a), (b) and (c)")


def _run_row(tag, att, img, label, key):
    """embedding_v2_BigGAN.py:78-165 in mode W at batch 1 on `img` [1,3,64,64] with `label`; freshly loaded G / E (the same weight_u /
    weight_v start for every row) and the noise feed `key` (the same for every row).  Returns the dict of this row's arrays."""
    from model.biggan_generator import BigGAN
    from model.utils.biggan_config import BigGANConfig
    import model.E.E_BIG as EBG
    import training_utils as TU
    from model.utils.custom_adam import LREQAdam
    from oracle import lpips_ref as LRF
    LP = LRF.seeded_params(0)
    lp = lambda a, b: LRF.lpips(LP, a, b)
    flat = lambda inf: [inf[0][0], inf[0][1], inf[0][2], inf[1], inf[2], inf[3], inf[4]]
    G = BigGAN(BigGANConfig.from_dict(GG.BIGGAN_SMALL_CFG))
    G.load_state_dict(R.fill_biggan(GG.shapes_of(G.state_dict()), seed=71))
    E = EBG.BE(startf=32, maxf=512, layer_count=5, biggan=True)
    E.load_state_dict(R.fill_encbig(GG.shapes_of(E.state_dict()), seed=81))
    gcpp, mask2cam = GB._attention() if att else (None, None)
    out = {}
    conditions = torch.tensor(TU.one_hot((np.array(label) * np.ones(1)).astype(np.int64)), dtype=torch.float)
    truncation = torch.tensor(0.4, dtype=torch.float)
    embed = G.embeddings(conditions)
    z0 = torch.tensor(TU.truncated_noise_sample(truncation=0.4, batch_size=1, seed=ITERATIONS % 30000), dtype=torch.float)
    cond_vector = torch.cat((z0, embed), dim=1)
    out["cond_vector"] = cond_vector.detach().clone()
    with GG._NoiseFeeder(f"{key}.{tag}.init", 2) as nf:
        const1, w1_ = E(img, cond_vector)
    out["init_noise_shapes"] = np.array([list(s_) for s_ in nf.log])
    w1 = w1_.detach()
    w1.requires_grad = True
    out["w0"] = w1.detach().clone()
    out["const1"] = const1.detach().clone()
    opt = LREQAdam([{"params": w1}], lr=LR, betas=(0.0, 0.99), weight_decay=0)
    for it in range(ITERATIONS):
        pre = f"it{it}_"
        with GG._NoiseFeeder(f"{key}.{tag}.it{it}", 2) as nf, warnings.catch_warnings():
            warnings.simplefilter("ignore")
            split = [nf.i]
            imgs2, _ = G(w1, conditions, truncation)
            const2, w2 = E(imgs2, cond_vector)
            split.append(nf.i)
            loss_imgs, i_imgs = TU.space_loss(img, imgs2, lpips_model=lp)
            loss_msiv = loss_imgs
            rows = [flat(i_imgs)]
            if att:
                with contextlib.redirect_stdout(io.StringIO()):
                    mask_1 = gcpp(img, None)
                    mask_2 = gcpp(imgs2, None)
                _, cam_1 = mask2cam(mask_1, img)
                _, cam_2 = mask2cam(mask_2, imgs2)
                mask_1, mask_2, cam_1, cam_2 = mask_1.float(), mask_2.float(), cam_1.float(), cam_2.float()
                loss_mask, i_mask = TU.space_loss(mask_1.detach().clone(), mask_2.detach().clone(), lpips_model=lp)
                loss_cam, i_cam = TU.space_loss(cam_1.detach().clone(), cam_2.detach().clone(), lpips_model=lp)
                loss_msiv = loss_imgs + loss_mask + loss_cam
                rows += [flat(i_mask), flat(i_cam)]
                out[pre + "mask_2"] = mask_2
                out[pre + "att_losses"] = np.array([float(loss_mask), float(loss_cam)])
            opt.zero_grad()
            loss_msiv.backward(retain_graph=True)
            out[pre + "grad1:w1"] = w1.grad.clone()
            opt.step()
            loss_w, i_w = TU.space_loss(w1, w2, image_space=False)
            loss_c2, i_c2 = TU.space_loss(const1, const2, image_space=False)
            loss_mslv = loss_w * 0.01
            opt.zero_grad()
            loss_mslv.backward(retain_graph=True)
            out[pre + "grad2:w1"] = w1.grad.clone()
            opt.step()
        if it == 0:
            out["noise_shapes"] = np.array([list(s_) for s_ in nf.log])
            out["noise_split"] = np.array(split)
        out[pre + "w1"] = w1.detach().clone()
        out[pre + "w2"] = w2.detach().clone()
        out[pre + "imgs2"] = imgs2.detach()[:, :, ::2, ::2].clone()        # every second pixel: keeps the file small
        out[pre + "imgs2_norm"] = imgs2.detach().norm()
        out[pre + "const2"] = const2.detach().clone()
        out[pre + "losses"] = np.array([float(loss_msiv), float(loss_imgs), float(loss_w), float(loss_c2), float(loss_mslv)])
        out[pre + "info"] = np.array(rows + [flat(i_w), flat(i_c2)])
        out[pre + "param_checksum"] = np.array(R.checksum({"w1": w1.detach()}))
        print(tag, "label", label, "it", it, out[pre + "losses"])
    return out


PER_RUN = ("init_noise_shapes", "noise_shapes", "noise_split")          # the same for every row: stored once


def gen_embed_v2_big_rows():
    GG._stub("boto3"); GG._stub("botocore"); GG._stub("botocore.exceptions", ClientError=Exception)
    GG._stub("requests")
    key = "embed_v2_big_rows"
    # the rows are scaled differently: their losses lie far apart, and far from the one loss of the coupled batch
    imgs1 = torch.tanh(R.randn(key + ".img", (len(LABELS), 3, 64, 64), 73, 0.8)) * torch.tensor(IMG_SCALES).view(-1, 1, 1, 1)
    out = {"imgs1": imgs1, "labels": np.array(LABELS)}
    for tag, att in (("W", False), ("W-att", True)):
        runs = [_run_row(tag, att, imgs1[b:b + 1], LABELS[b], key) for b in range(len(LABELS))]
        for k in runs[0]:
            vals = [torch.as_tensor(np.asarray(r_[k].detach() if torch.is_tensor(r_[k]) else r_[k])) for r_ in runs]
            if k in PER_RUN:
                assert all(torch.equal(v, vals[0]) for v in vals), k
                out[f"{tag}_{k}"] = vals[0]
            elif vals[0].dim() and vals[0].shape[0] == 1 and k not in ("it0_info", "it1_info"):
                out[f"{tag}_{k}"] = torch.cat(vals)               # [1, ...] per run -> [B, ...]
            else:
                out[f"{tag}_{k}"] = torch.stack(vals)             # scalars and per-run tables -> a leading B
    GG.save_npz("embed_v2_big_rows.npz", **out)


SECTIONS = {"gradcam_rows": gen_gradcam_rows, "embed_v2_big_rows": gen_embed_v2_big_rows}

if __name__ == "__main__":
    for s_ in sys.argv[1:] or list(SECTIONS):
        print("==", s_)
        SECTIONS[s_]()
