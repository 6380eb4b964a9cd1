#!/usr/bin/env python3
"""Golden vectors for the masked projection (dge_amd.projector with a mask) from the reference's own generator.

Runs ONLY in the build container (needs the reference tree; a no-op elsewhere).  Imports the reference modules (never copies them)
through tools/gen_golden.py's stubs and helpers; writes tests/golden/projector_mask.npz only.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_projector_mask.py

projector_mask.npz: tools/gen_golden_projector.py's loop - the same model, targets, z samples and w-noise draws, B = 2, three
iterations - with the distance replaced by the float64 restatement of the masked LPIPS (tests/masked_lpips_ref.py) under the fixed
soft-edged half-plane mask of tests/projector_mask_models.py.  The generator, the regulariser and Adam stay in f32; the image is
cast to float64 for the distance and the gradient comes back through the cast.  Stored: the mask and, per iteration, dist [B],
reg [B], the gradients of w and of the maps and w and the maps behind the step and the renormalisation; z, w_avg, w_std, the
targets, the w noise, lr and noise_scale are projector.npz's and are not stored again.

Data only.  The loop runs twice and the file is written only when the two runs agree bit for bit, and only when no more than
EXEMPT_CAP of any tensor's gradient lies below EXEMPT_BELOW of its largest (tests/projector_models.py): the GPU parity test may
leave such elements out, and the mask was chosen so that the reference run alone stays inside the cap.
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG          # noqa: E402  (exits when the reference is absent; installs the torchvision / PIL stubs)

import numpy as np               # noqa: E402
import torch                     # noqa: E402

from gen_golden_projector import schedule           # noqa: E402
from gen_golden_s2_noise import projector_reg        # noqa: E402
from tests.masked_lpips_ref import masked_lpips, params64          # noqa: E402
from tests.projector_mask_models import proj_mask   # noqa: E402
from tests.projector_models import (EXEMPT_BELOW, EXEMPT_CAP, PROJ_B, PROJ_ITERS, PROJ_KW, PROJ_SETTINGS, exempt_mask, proj_state_dict,   # noqa: E402
                                     proj_targets, proj_w_noise, proj_z, split_maps)
from tests.s2_noise_models import S2N_RES           # noqa: E402


def run():
    from model.stylegan2_generator import StyleGAN2Generator
    from oracle import lpips_ref as LRF
    torch.set_num_threads(1)
    S, B = PROJ_SETTINGS, PROJ_B
    G = StyleGAN2Generator(64, **PROJ_KW)
    G.load_state_dict(proj_state_dict())
    G.eval()
    for p_ in G.parameters():
        p_.requires_grad_(False)
    LP = params64(LRF.seeded_params(0))
    layers = [getattr(G.synthesis, f"layer{i}") for i in range(len(S2N_RES))]
    target, mask = proj_targets(), proj_mask()
    with torch.no_grad():
        ws = G.mapping(proj_z())["w"]
    w_avg = ws.mean(dim=0)
    w_std = float((((ws.double() - ws.double().mean(dim=0)) ** 2).sum() / ws.shape[0]).sqrt())
    out = dict(mask=mask)
    w = w_avg.reshape(1, -1).repeat(B, 1).clone().requires_grad_(True)
    maps = []
    for L in layers:          # a copy of the buffer per row, as leaves
        L._buffers["noise"] = L.noise.detach().reshape(1, 1, L.res, L.res).repeat(B, 1, 1, 1).clone().requires_grad_(True)
        maps.append(L.noise)
    opt = torch.optim.Adam([w] + maps, lr=S["lr"], betas=(0.9, 0.999))
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).clone()
    for it in range(PROJ_ITERS):
        lr_t, ns = schedule(it, S)
        for g in opt.param_groups:
            g["lr"] = lr_t
        scale = torch.tensor(w_std * ns, dtype=torch.float32)
        wp = (w + proj_w_noise(it) * scale).unsqueeze(1).repeat(1, G.num_layers, 1)
        img = G.synthesis(wp, randomize_noise=False)["image"]
        dist = masked_lpips(LP, target.double(), img.double(), mask.double()).reshape(B)
        reg = torch.stack([sum(projector_reg(n[b:b + 1]) for n in maps) for b in range(B)])
        opt.zero_grad()
        (dist.sum() + (S["noise_reg"] * reg.sum()).double()).backward()
        pre = f"it{it}"
        out[f"{pre}_dist"], out[f"{pre}_reg"] = dist.detach().float().clone(), reg.detach().clone()
        out[f"{pre}_w_grad"], out[f"{pre}_noise_grad"] = w.grad.clone(), cat([n.grad for n in maps])
        opt.step()
        with torch.no_grad():
            for n in maps:
                n -= n.mean(dim=(1, 2, 3), keepdim=True)
                n *= n.square().mean(dim=(1, 2, 3), keepdim=True).rsqrt()
        out[f"{pre}_w"], out[f"{pre}_noise"] = w.detach().clone(), cat(maps)
        print("it", it, "lr", lr_t, "dist", dist.tolist(), "reg", reg.tolist())
    return {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}


if __name__ == "__main__":
    a, b = run(), run()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f"{k} differs between two runs"
    print("two runs agree bit for bit")
    for it in range(PROJ_ITERS):
        for k, x in enumerate([a[f"it{it}_w_grad"]] + split_maps(a[f"it{it}_noise_grad"])):
            share = float(exempt_mask(x).mean())
            assert share <= EXEMPT_CAP, f"iteration {it}, tensor {k}: {share} of the gradient lies below {EXEMPT_BELOW} of its largest"
    GG.save_npz("projector_mask.npz", **a)
