#!/usr/bin/env python3
"""Golden vectors for the StyleSpace codes of StyleGAN2 (dge_amd.style_codes, synthesis(styles=...), projector.StyleProjectorStep)
from the reference's own generator.

Runs ONLY in the build container (needs the reference tree; a no-op elsewhere).  Imports the reference modules (never copies them)
through tools/gen_golden.py's stubs and helpers; writes under tests/golden/ only.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_s2_styles.py

The reference's ModulateConvBlock.forward calls `self.style(w)`.  A forward hook on every `style` module that returns a leaf tensor
in place of the module's output makes the style vectors inputs of the reference's graph: its autograd then yields
d<image, gimg> / d styles, and an optimiser over the leaves runs the S refinement.

s2_styles.npz          : the 64^2 generator of tests/s2_noise_models.py (noise strengths away from 0), B = 2: wp, gimg, the image,
                         the styles and g_styles, both in the flat layout of style_codes.style_layout (block g as [B,C_g] at
                         B * off_g; conv blocks first, then the toRGB blocks); `param:` entries: the conv biases moved off the
                         leaky-relu kink for this forward (GG.clear_kinks, for the reason the README gives), `kink_margin`.
projector_styles.npz   : three iterations of StyleProjectorStep's loop composed from the reference's generator
                         (tests/projector_models.py) with the hooks' leaves and its noise buffers as leaves (a copy per row),
                         torch.optim.Adam(betas=(0.9, 0.999)) over the style leaves + maps, the projector's noise regulariser and
                         the seeded LPIPS stand-in, as tools/gen_golden_projector.py composes the W loop.  B = 2, f32, steps = 20,
                         base rate 0.01.  Stored: the start wp, the target, and per iteration lr, dist [B], reg [B], the gradients
                         of the styles and of the maps, and the styles and maps behind the step and the renormalisation.

Data only.  Every input is seeded by name (tests/golden/recipe.py) and every sum runs on one thread; the tool runs everything twice
and refuses to write unless the two runs agree bit for bit.
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG          # noqa: E402  (exits when the reference is absent; installs the torchvision / PIL stubs)

import numpy as np               # noqa: E402
import torch                     # noqa: E402

from gen_golden_projector import schedule        # noqa: E402
from gen_golden_s2_noise import projector_reg    # noqa: E402
from tests.golden import recipe as R             # noqa: E402
from tests.projector_models import PROJ_B, PROJ_ITERS, PROJ_KW, proj_state_dict, proj_targets, proj_z        # noqa: E402
from tests.s2_noise_models import S2N_KW, S2N_RES, s2n_state_dict        # noqa: E402
from tests.s2_style_models import STYLE_SETTINGS, style_start_wp, styles_wp_gimg        # noqa: E402

NL = len(S2N_RES) + 1          # rows of wp at 64^2


def style_modules(G):
    """[(style DenseBlock, its row of wp)] in the order of the flat style buffer: the conv blocks, then the toRGB blocks."""
    syn = G.synthesis
    return [(getattr(syn, f"layer{i}").style, i) for i in range(NL - 1)] + [(getattr(syn, f"output{k}").style, 2 * k + 1) for k in range(NL // 2)]


def hook_styles(G, leaves):
    """Every style module returns its leaf [B,C_g] instead of its output; -> the hooks' handles."""
    return [m.register_forward_hook(lambda mod, inp, out, leaf=leaf: leaf) for (m, _), leaf in zip(style_modules(G), leaves)]


def flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]).clone()


def _generator(sd, kw):
    from model.stylegan2_generator import StyleGAN2Generator
    G = StyleGAN2Generator(64, **kw)
    G.load_state_dict(sd)
    G.eval()
    for p_ in G.parameters():
        p_.requires_grad_(False)
    return G


def run_s2_styles():
    torch.set_num_threads(1)
    G = _generator(s2n_state_dict(), S2N_KW)
    wp, gimg = styles_wp_gimg()
    layers = [getattr(G.synthesis, f"layer{i}") for i in range(NL - 1)]
    nudged, margin = GG.clear_kinks([lambda: G.synthesis(wp, randomize_noise=False)], [L.bias for L in layers],
                                    [f"synthesis.layer{i}.bias" for i in range(NL - 1)])
    out = {"param:" + k: v for k, v in nudged.items()}
    out["kink_margin"] = np.array(margin)
    with torch.no_grad():
        plain = G.synthesis(wp, randomize_noise=False)["image"]
        leaves = [m(wp[:, row]).detach().clone().requires_grad_(True) for m, row in style_modules(G)]
    handles = hook_styles(G, leaves)
    img = G.synthesis(wp, randomize_noise=False)["image"]
    for h in handles:
        h.remove()
    assert torch.equal(img.detach(), plain), "the hooked forward differs from the plain one"
    (img * gimg).sum().backward()
    out.update(wp=wp, gimg=gimg, image=img.detach(), styles=flat(leaves), g_styles=flat([s_.grad for s_ in leaves]))
    return {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}


def run_projector_styles():
    from oracle import lpips_ref as LRF
    torch.set_num_threads(1)
    S, B = STYLE_SETTINGS, PROJ_B
    G = _generator(proj_state_dict(), PROJ_KW)
    LP = LRF.seeded_params(0)
    layers = [getattr(G.synthesis, f"layer{i}") for i in range(NL - 1)]
    target = proj_targets()
    with torch.no_grad():
        wp = style_start_wp(G.mapping(proj_z()[:B])["w"], NL)
        leaves = [m(wp[:, row]).detach().clone().requires_grad_(True) for m, row in style_modules(G)]
    hook_styles(G, leaves)
    maps = []
    for L in layers:          # a copy of the buffer per row, as leaves
        L._buffers["noise"] = L.noise.detach().reshape(1, 1, L.res, L.res).repeat(B, 1, 1, 1).clone().requires_grad_(True)
        maps.append(L.noise)
    out = dict(wp=wp, target=target, styles0=flat(leaves))
    opt = torch.optim.Adam(leaves + maps, lr=S["lr"], betas=(0.9, 0.999))
    for it in range(PROJ_ITERS):
        lr_t, _ = schedule(it, dict(S, initial_noise_factor=0.0, noise_ramp=1.0))
        for g in opt.param_groups:
            g["lr"] = lr_t
        img = G.synthesis(wp, randomize_noise=False)["image"]          # (wp only sets the batch: every style comes from its leaf)
        dist = LRF.lpips(LP, target, img).reshape(B)
        reg = torch.stack([sum(projector_reg(n[b:b + 1]) for n in maps) for b in range(B)])
        opt.zero_grad()
        (dist.sum() + S["noise_reg"] * reg.sum()).backward()
        pre = f"it{it}"
        out[f"{pre}_lr"] = np.array(lr_t)
        out[f"{pre}_dist"], out[f"{pre}_reg"] = dist.detach().clone(), reg.detach().clone()
        out[f"{pre}_style_grad"], out[f"{pre}_noise_grad"] = flat([s_.grad for s_ in leaves]), flat([n.grad for n in maps])
        opt.step()
        with torch.no_grad():
            for n in maps:
                n -= n.mean(dim=(1, 2, 3), keepdim=True)
                n *= n.square().mean(dim=(1, 2, 3), keepdim=True).rsqrt()
        out[f"{pre}_styles"], out[f"{pre}_noise"] = flat(leaves), flat(maps)
        print("it", it, "lr", lr_t, "dist", dist.tolist(), "reg", reg.tolist())
    return {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}


def twice(run):
    a, b = run(), run()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f"{k} differs between two runs"
    return a


if __name__ == "__main__":
    a, b = twice(run_s2_styles), twice(run_projector_styles)
    print("two runs agree bit for bit")
    GG.save_npz("s2_styles.npz", **a)
    GG.save_npz("projector_styles.npz", **b)
