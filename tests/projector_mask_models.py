"""What the masked-projector tests and tools/gen_golden_projector_mask.py share beyond tests/projector_models.py: the fixture's
mask."""
import torch

from tests.projector_models import PROJ_B


def proj_mask(B=PROJ_B, res=64):
    """[B,1,res,res] f32: a soft-edged half-plane, 1 on the left, a linear ramp of res/4 columns to 0 on the right; row b's edge
    sits b * res/8 columns further right, so the rows of a group differ."""
    x = torch.arange(res, dtype=torch.float32)
    rows = [((res * 0.5 + b * res / 8 + res / 8 - x) / (res / 4)).clamp(0, 1).view(1, 1, res).expand(1, res, res) for b in range(B)]
    return torch.stack(rows).contiguous()
