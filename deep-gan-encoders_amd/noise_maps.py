"""The optimised noise maps of StyleGAN2's synthesis, owned once for embedding_v2.LatentEmbedStep and projector.ProjectorStep."""
import os

import torch

from . import ops


class NoiseMaps:
    """The maps of `synthesis`'s conv layers in one flat f32 leaf `flat` (layout: the ops.NoiseTable `table`; Bn rows per map, 1 = one
    set shared by the batch), the flat gradient buffer `gflat`, the per-layer leaves `maps` with their gradient views `grads`, and the
    regulariser's value per row `reg` [Bn], all allocated here (a captured iteration keeps the addresses).  The optimiser is the step's."""

    def __init__(self, synthesis, Bn, device):
        self.layers = [getattr(synthesis, f"layer{i}") for i in range(synthesis.num_layers - 1)]
        tab = self.table = ops.NoiseTable([L.res for L in self.layers], Bn, device)
        self.flat = torch.zeros(tab.numel, dtype=torch.float32, device=device, requires_grad=True)
        self.gflat = torch.zeros(tab.numel, dtype=torch.float32, device=device)
        self.reg = torch.zeros(Bn, dtype=torch.float32, device=device)
        # the maps the generator sees: leaves of their own on the flat storage (their gradients go to the views of gflat)
        self.maps = [tab.view(self.flat.detach(), m).requires_grad_(True) for m in range(len(self.layers))]
        self.grads = [tab.view(self.gflat, m) for m in range(len(self.layers))]

    def fits(self, Bn, device):          # whether this allocation serves a group with Bn rows per map on `device`
        return self.table.Bn == Bn and self.table.device == torch.device(device)

    def reset(self):
        """Every row of every map = the generator's `layer{i}.noise` buffer, in place."""
        with torch.no_grad():
            for m, L in zip(self.maps, self.layers):
                m.copy_(L.noise.reshape(1, L.res, L.res).expand_as(m))

    def add_reg(self, scale):
        """-> reg, the regulariser of every row (dge_noise_reg); `scale` times its gradient is ADDED to gflat."""
        return ops.noise_reg(self.table, self.flat.detach(), grad=self.gflat, scale=scale, accumulate=True, out=self.reg)

    def hand_grad(self):
        self.flat.grad = self.gflat          # what the optimiser over `flat` reads

    def normalize(self):          # every row of every map to zero mean and unit mean square
        ops.noise_normalize(self.table, self.flat.detach())

    def detached(self):
        return [m.detach() for m in self.maps]


def save_noise_rows(maps, rows, numbers, models_dir):
    """models_dir/id{n}-noise.pt for every pair (row b, number n): row b of every map, each [1,res,res], as synthesis(noises=...) takes them."""
    for b, n in zip(rows, numbers):
        torch.save([m[b:b + 1].clone() for m in maps], os.path.join(models_dir, "id%d-noise.pt" % n))
