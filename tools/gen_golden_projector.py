#!/usr/bin/env python3
"""Golden vectors for StyleGAN2's projector (dge_amd.projector) from the reference's own generator.

Runs ONLY in the build container (needs the reference tree; a no-op elsewhere).  Imports the reference modules (never copies them)
through tools/gen_golden.py's stubs and helpers; writes tests/golden/projector.npz only.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_projector.py

projector.npz: three iterations of the loop of dge_amd/projector.py's docstring, composed from the reference's StyleGAN2Generator at
64^2 (tests/projector_models.py) with its noise buffers as leaves (a copy per row, [B,1,R,R]), torch.optim.Adam(betas=(0.9, 0.999))
over [w] + maps, the projector's noise regulariser written with avg_pool2d / torch.roll (as tests/test_noise_reg_ref.py ties it) and
the seeded LPIPS stand-in (oracle/lpips_ref.py, the restatement embed_v2_noise.npz used).  B = 2, f32, w_avg_samples = 64,
steps = 20: the schedule moves between the iterations.  Stored: the z samples, w_avg, w_std, the target images, the w-noise
draws and, per iteration, lr and noise_scale, dist [B], reg [B], the gradients of w and of the maps
(concatenated in layer order, each [B,R,R]) and w and the maps behind the step and the renormalisation.

Data only.  Every input is seeded by name (tests/golden/recipe.py) and every sum runs on one thread, so a second run reproduces the
file's arrays bit for bit; the tool checks that itself by running the loop twice before it writes.
"""
import math
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG          # noqa: E402  (exits when the reference is absent; installs the torchvision / PIL stubs)

import numpy as np               # noqa: E402
import torch                     # noqa: E402

from gen_golden_s2_noise import projector_reg        # noqa: E402
from tests.projector_models import PROJ_B, PROJ_ITERS, PROJ_KW, PROJ_SETTINGS, proj_state_dict, proj_targets, proj_w_noise, proj_z   # noqa: E402
from tests.s2_noise_models import S2N_RES           # noqa: E402


def schedule(step, S):
    """StyleGAN2's projector: (learning rate, w-noise scale / w_std) of iteration `step`."""
    t = step / S["steps"]
    noise = S["initial_noise_factor"] * max(0.0, 1.0 - t / S["noise_ramp"]) ** 2
    r = min(1.0, (1.0 - t) / S["lr_rampdown"])
    r = 0.5 - 0.5 * math.cos(r * math.pi)
    r = r * min(1.0, t / S["lr_rampup"])
    return S["lr"] * r, noise


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
    LP = LRF.seeded_params(0)
    layers = [getattr(G.synthesis, f"layer{i}") for i in range(len(S2N_RES))]
    target = proj_targets()
    z = proj_z()
    with torch.no_grad():
        ws = G.mapping(z)["w"]
    w_avg = ws.mean(dim=0)
    w_std = float((((ws.double() - ws.double().mean(dim=0)) ** 2).sum() / ws.shape[0]).sqrt())
    out = dict(z=z, w_avg=w_avg, w_std=np.array(w_std), target=target)
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
        wn = proj_w_noise(it)
        scale = torch.tensor(w_std * ns, dtype=torch.float32)          # (the f32 scalar the device multiplies by)
        wp = (w + wn * scale).unsqueeze(1).repeat(1, G.num_layers, 1)
        img = G.synthesis(wp, randomize_noise=False)["image"]
        dist = LRF.lpips(LP, target, img).reshape(B)
        reg = torch.stack([sum(projector_reg(n[b:b + 1]) for n in maps) for b in range(B)])
        opt.zero_grad()
        (dist.sum() + S["noise_reg"] * reg.sum()).backward()
        pre = f"it{it}"
        out[f"{pre}_lr"], out[f"{pre}_noise_scale"] = np.array(lr_t), np.array(float(scale))
        out[f"{pre}_w_noise"] = wn
        out[f"{pre}_dist"], out[f"{pre}_reg"] = dist.detach().clone(), reg.detach().clone()
        out[f"{pre}_w_grad"], out[f"{pre}_noise_grad"] = w.grad.clone(), cat([n.grad for n in maps])
        opt.step()
        with torch.no_grad():
            for n in maps:
                n -= n.mean(dim=(1, 2, 3), keepdim=True)
                n *= n.square().mean(dim=(1, 2, 3), keepdim=True).rsqrt()
        out[f"{pre}_w"], out[f"{pre}_noise"] = w.detach().clone(), cat(maps)
        print("it", it, "lr", lr_t, "scale", float(scale), "dist", dist.tolist(), "reg", reg.tolist())
    return {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}


if __name__ == "__main__":
    a, b = run(), run()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f"{k} differs between two runs"
    print("two runs agree bit for bit")
    GG.save_npz("projector.npz", **a)
