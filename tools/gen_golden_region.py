#!/usr/bin/env python3
"""Golden vectors for the region directions of StyleGAN2 (dge_amd.region_directions) from the reference's own generator.

Runs ONLY in the build container (needs the reference tree; a no-op elsewhere).  Imports the reference modules (never copies them)
through tools/gen_golden.py's stubs and helpers; writes tests/golden/region.npz only.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_region.py

region.npz: the reference's StyleGAN2Generator at 64^2 (tests/region_models.py), one seeded z -> wp, K = 16 seeded orthonormal axes
Q (QR in float64), every W+ row moved, h = 0.25, 2 x 2 pooling, reg = 1e-3, two rectangular masks (even bounds; odd bounds, whose
pooled weights take 0.25 and 0.5).  Stored: Q, wp, the masks; from the generator in float64 the finite-difference operand X [16, 3072],
M_f / M_b per mask and the solve of tests/region_ref.py (eps, ratio, coefficient vectors); M_f / M_b from the generator run in f32,
their errors e_ref = max |M32 - M64| / max |M64| and the relative eigenvalue error lam_err_ref of the solve on them; the float64
Grams of the exact autograd Jacobian and the truncation they document.

Data only.  Every input is seeded by name and every sum runs on one thread; the tool runs everything twice and refuses to write
unless the two runs agree bit for bit, and refuses when fewer than three ratios of a mask are separated by REGION_GAP.
"""
import copy
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG          # noqa: E402  (exits when the reference is absent; installs the torchvision / PIL stubs)

import numpy as np               # noqa: E402
import torch                     # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tests import region_ref as RR          # noqa: E402
from tests.region_models import (REGION_GAP, REGION_K, REGION_KW, REGION_POOL, REGION_REG, REGION_ROWS, REGION_STEP, region_basis,
                                 region_masks, region_state_dict, region_z)          # noqa: E402


def fd_operand(G, wp, Q, dtype):
    """X [K, 3 (H/s)^2] in `dtype`: row k = (pool(I(wp + h q_k)) - pool(I(wp - h q_k))) / (2h) on rows REGION_ROWS"""
    h, s = REGION_STEP, REGION_POOL
    r0, r1 = REGION_ROWS
    wp, Q = wp.to(dtype), Q.to(dtype)
    rows = []
    with torch.no_grad():
        for k in range(Q.shape[0]):
            pair = wp.repeat(2, 1, 1)
            pair[0, r0:r1] = wp[0, r0:r1] + h * Q[k]
            pair[1, r0:r1] = wp[0, r0:r1] - h * Q[k]
            img = F.avg_pool2d(G.synthesis(pair, randomize_noise=False)["image"], s)
            rows.append(((img[0] - img[1]) / (2 * h)).reshape(-1))
    return torch.stack(rows)


def exact_operand(G, wp, Q):
    """The autograd Jacobian of the pooled float64 image with respect to the coefficients along Q, as X [K, N]"""
    r0, r1 = REGION_ROWS
    wp, Q = wp.double(), Q.double()
    t = torch.zeros(Q.shape[0], dtype=torch.float64, requires_grad=True)
    code = wp.clone()
    code = torch.cat((code[:, :r0], code[:, r0:r1] + (t @ Q)[None, None], code[:, r1:]), dim=1)
    out = F.avg_pool2d(G.synthesis(code, randomize_noise=False)["image"], REGION_POOL).reshape(-1)
    eye = torch.eye(out.numel(), dtype=torch.float64)
    J, = torch.autograd.grad(out, t, eye, is_grads_batched=True)          # [N, K]
    return J.t().contiguous()


def run():
    from model.stylegan2_generator import StyleGAN2Generator
    torch.set_num_threads(1)
    G = StyleGAN2Generator(64, **REGION_KW)
    G.load_state_dict(region_state_dict())
    G.eval()
    for p_ in G.parameters():
        p_.requires_grad_(False)
    G64 = copy.deepcopy(G).double()
    Q, masks = region_basis(), region_masks()
    with torch.no_grad():
        w = G.mapping(region_z())["w"]
    wp = w.reshape(1, 1, -1).repeat(1, G.num_layers, 1).contiguous()
    X64 = fd_operand(G64, wp, Q, torch.float64).numpy()
    X32 = fd_operand(G, wp, Q, torch.float32)
    XJ = exact_operand(G64, wp, Q).numpy()
    out = dict(Q=Q, wp=wp, masks=masks, X=X64, step=np.array(REGION_STEP), pool=np.array(REGION_POOL), reg=np.array(REGION_REG),
               rows=np.array(REGION_ROWS))
    for i in range(masks.shape[0]):
        mu = RR.pooled_weights(masks[i, 0].numpy(), REGION_POOL)
        Mf, Mb = RR.grams_ref(X64, mu)
        w32 = torch.from_numpy(np.tile(mu, X32.shape[1] // len(mu)).astype(np.float32))          # (0, 0.25, 0.5, 1: exact in f32)
        Mf32, Mb32 = ((X32 * w32) @ X32.t()).numpy(), ((X32 * (1.0 - w32)) @ X32.t()).numpy()
        Jf, Jb = RR.grams_ref(XJ, mu)
        eps, lam, c, d = RR.solve_ref(Mf, Mb, REGION_REG, Q.numpy())
        _, lam32, _, _ = RR.solve_ref(Mf32, Mb32, REGION_REG, Q.numpy())
        gaps = RR.rel_gaps(lam)
        e_ref = np.array([np.abs(Mf32 - Mf).max() / np.abs(Mf).max(), np.abs(Mb32 - Mb).max() / np.abs(Mb).max()])
        trunc = np.array([np.abs(Mf - Jf).max() / np.abs(Jf).max(), np.abs(Mb - Jb).max() / np.abs(Jb).max()])
        pre = f"m{i}_"
        out.update({pre + "mu": mu, pre + "M_f": Mf, pre + "M_b": Mb, pre + "M_f32": Mf32, pre + "M_b32": Mb32, pre + "J_f": Jf, pre + "J_b": Jb,
                    pre + "eps": np.array(eps), pre + "ratio": lam, pre + "coeffs": c, pre + "directions": d, pre + "e_ref": e_ref,
                    pre + "lam_err_ref": np.array(np.abs(lam32 - lam).max() / lam[0]), pre + "truncation": trunc, pre + "gaps": gaps})
        print(f"mask {i}: ratio[:6] {lam[:6]}  separated {int((gaps >= REGION_GAP).sum())}  e_ref {e_ref}  lam_err_ref "
              f"{float(out[pre + 'lam_err_ref']):.3e}  truncation {trunc}")
    return {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}


if __name__ == "__main__":
    a, b = run(), run()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f"{k} differs between two runs"
    print("two runs agree bit for bit")
    for i in range(a["masks"].shape[0]):
        n = int((a[f"m{i}_gaps"] >= REGION_GAP).sum())
        assert n >= 3, f"mask {i}: only {n} ratios are separated by {REGION_GAP}: the vector checks would have too little to hold on to"
    assert REGION_K == a["Q"].shape[0]
    GG.save_npz("region.npz", **a)
