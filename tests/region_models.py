"""What the region-direction tests and tools/gen_golden_region.py share: the 64^2 StyleGAN2 model of tests/projector_models.py
(noise strengths away from 0, the mapping network at a real checkpoint's scale), the run's settings and its seeded inputs."""
import functools
import os

import numpy as np
import torch

from tests.golden import recipe as R
from tests.projector_models import PROJ_KW, proj_state_dict

REGION_KW = PROJ_KW
REGION_SIZE, REGION_L = 64, 10
REGION_K = 16                        # axes of the seeded orthonormal basis
REGION_ROWS = (0, 10)                # the W+ rows [r0, r1) that move: every row of the 64^2 model
REGION_STEP, REGION_POOL, REGION_REG = 0.25, 2, 1e-3
REGION_JAC_RES = REGION_SIZE // REGION_POOL
REGION_GAP = 0.02                    # a ratio counts as separated when its relative gap min_j |l_k - l_j| / l_0 is at least this
# (y0, y1, x0, x1) of the white rectangles: even bounds (the pooled weights are 0 and 1), odd bounds (the pooled weights take 0.5 on
# the edges and 0.25 at the corners)
REGION_RECTS = ((16, 40, 20, 48), (15, 41, 21, 47))
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "region.npz")


def region_state_dict():
    return proj_state_dict()


def region_z():
    return R.randn("region.z", (1, 512), 91)


def region_basis():
    """Q [K,512] f32: the orthonormal columns of a QR factorisation in float64 of a seeded normal matrix, as rows"""
    A = R.randn("region.basis", (512, REGION_K), 92).double().numpy()
    Q, _ = np.linalg.qr(A)
    return torch.from_numpy(np.ascontiguousarray(Q.T).astype(np.float32))


def region_masks():
    """[2,1,64,64] f32: the two rectangles"""
    m = torch.zeros(len(REGION_RECTS), 1, REGION_SIZE, REGION_SIZE)
    for i, (y0, y1, x0, x1) in enumerate(REGION_RECTS):
        m[i, 0, y0:y1, x0:x1] = 1.0
    return m


@functools.lru_cache(maxsize=None)
def fixture():
    """region.npz as a dict of read-only arrays, loaded once per process"""
    with np.load(FIXTURE) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out
