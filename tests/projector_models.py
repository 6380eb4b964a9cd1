"""What the projector tests and tools/gen_golden_projector.py share: the 64^2 StyleGAN2 model (tests/s2_noise_models.py: noise
strengths away from 0; tests/s2z_models.py: the mapping network at a real checkpoint's scale), the run's settings and its seeded
inputs; and what the CPU and the GPU test file share about the fixture's gradients."""
import numpy as np
import torch

from tests.golden import recipe as R
from tests.s2_noise_models import S2N_KW, S2N_RES, noise_strength
from tests.s2z_models import s2z_state_dict

PROJ_KW = S2N_KW
PROJ_B, PROJ_ITERS = 2, 3
PROJ_SETTINGS = dict(steps=20, lr=0.1, initial_noise_factor=0.05, noise_ramp=0.75, lr_rampdown=0.25, lr_rampup=0.05, noise_reg=1e5,
                     w_avg_samples=64)


def proj_state_dict():
    sd = s2z_state_dict()
    for i in range(len(S2N_RES)):
        sd[f"synthesis.layer{i}.noise_strength"] = torch.tensor(noise_strength(i), dtype=torch.float32)
    return sd


def proj_targets():
    """The fixture's target images [PROJ_B,3,64,64] in (-1, 1)."""
    return torch.tanh(R.randn("projector.img", (PROJ_B, 3, 64, 64), 81, 0.8))


def proj_z():
    return R.randn("projector.z", (PROJ_SETTINGS["w_avg_samples"], 512), 82)


def proj_w_noise(it, n=PROJ_B, tag="projector"):
    return R.randn(f"{tag}.it{it}.wnoise", (n, 512), 83)


# Adam's first steps follow the sign of the gradient: an element whose fixture gradient is below EXEMPT_BELOW of its tensor's
# largest may step the other way.  The GPU parity test may leave such elements out, at most EXEMPT_CAP of any tensor
# (tests/test_projector_cli.py checks on the fixture that the reference's own gradients stay inside the cap).
EXEMPT_BELOW, EXEMPT_CAP = 1e-6, 1e-3


def exempt_mask(ref):
    """True where the fixture's gradient is below EXEMPT_BELOW of the tensor's largest"""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    return ref < EXEMPT_BELOW * ref.max()


def split_maps(flat, B=PROJ_B):
    """The flat layer-order buffer -> one [B,R,R] array per map"""
    out, off = [], 0
    for r in S2N_RES:
        out.append(np.asarray(flat[off:off + B * r * r]).reshape(B, r, r))
        off += B * r * r
    assert off == len(flat)
    return out
