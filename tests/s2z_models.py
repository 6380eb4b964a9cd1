"""Seeded StyleGAN2-64 weights of the z-gradient fixtures (s2_mapping_grad.npz, embed_v2_z.npz): the model of s2_small.npz with the
mapping network at the scale of a real checkpoint - weights N(0, 1) / lr_mul, so that w = O(1) and d w / d z is far above rounding
(recipe.fill_s2 leaves them at N(0, 1): w ~ 1e-2 and a z gradient of 1e-15)."""
from tests.golden import recipe as R
from tests.helpers import s2_shapes

S2Z_KW = dict(fmaps_base=2048, fmaps_max=128)
MAPPING_LR_MUL = 0.01


def s2z_state_dict():
    shapes = s2_shapes(64, **S2Z_KW)
    sd = R.fill_s2(shapes, seed=11)
    for k, shp in shapes.items():
        if k.startswith("mapping.") and k.endswith(".weight"):
            sd[k] = R.randn("s2z." + k, tuple(shp), 12, 1.0 / MAPPING_LR_MUL)
        elif k.startswith("mapping.") and k.endswith(".bias"):
            sd[k] = R.randn("s2z." + k, tuple(shp), 12, 0.1 / MAPPING_LR_MUL)
    return sd
