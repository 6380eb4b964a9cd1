"""What the StyleSpace tests and tools/gen_golden_s2_styles.py share: the seeded inputs of the two fixtures, the settings of the S
stage's run, and the flat layout of the style codes at 64^2 stated on its own (tests/s2_noise_models.py: fmaps_base 2048, fmaps_max
128)."""
import numpy as np
import torch

from tests.golden import recipe as R

STYLE_SETTINGS = dict(steps=20, lr=0.01, lr_rampdown=0.25, lr_rampup=0.05, noise_reg=1e5)
# the input channels of the modulated blocks at 64^2: conv layers 0 .. 8 (4^2: 128; 8^2, 16^2: 128; 32^2: 64; 64^2: 32; an up
# layer reads the resolution below), then the toRGB blocks 0 .. 4
S64_CONV = (128, 128, 128, 128, 128, 128, 64, 64, 32)
S64_RGB = (128, 128, 128, 64, 32)
S64_CHANNELS = S64_CONV + S64_RGB
S64_NAMES = tuple(f"layer{i}" for i in range(9)) + tuple(f"output{k}" for k in range(5))
S64_ROWS = tuple(range(9)) + (1, 3, 5, 7, 9)          # the row of wp that drives each block


def styles_wp_gimg():
    """s2_styles.npz: wp [2,10,512] and the cotangent of the image."""
    return R.randn("s2s.wp", (2, 10, 512), 5), R.randn("s2s.gimg", (2, 3, 64, 64), 5, 1.0 / (2 * 3 * 64 * 64) ** 0.5)


def style_start_wp(w, L):
    """projector_styles.npz: the start code of the S stage, w [B,512] of mapped samples in every row of W+ (what a W run leaves)."""
    return w.detach().unsqueeze(1).repeat(1, L, 1).contiguous()


def split_blocks(flat, B, channels=S64_CHANNELS):
    """The flat style buffer -> one [B,C_g] array per block"""
    out, off = [], 0
    for C in channels:
        out.append(np.asarray(flat[B * off:B * (off + C)]).reshape(B, C))
        off += C
    assert B * off == len(flat), (B * off, len(flat))
    return out
