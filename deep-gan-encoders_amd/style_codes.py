"""The StyleSpace (S) codes of StyleGAN2's synthesis network as an input of their own: the per-channel style vectors of the 17 conv
layers and the 9 toRGB blocks (StyleGAN2-1024: 6048 + 3040 = 9088 numbers per image), which `synthesis(wp)` only ever forms as an
intermediate.  Owned once, for synthesis(styles=...), projector.StyleProjectorStep and the files `id{n}-s.pt`."""
import torch

from .autograd_s2 import style_groups, styles_from_wp


def style_layout(synthesis, B):
    """(names, channels, offsets, total) of the flat style buffer for batch B - the layout autograd_s2._style_tables gives s_all:
    the conv blocks `layer0` .. first, then the toRGB blocks `output0` ..; block g holds [B,C_g] at float offset B * off_g, off_g the
    channels of the blocks in front of it; total = B * sum C_g."""
    nl = synthesis.num_layers
    names = [f"layer{i}" for i in range(nl - 1)] + [f"output{k}" for k in range(nl // 2)]
    channels = [L.in_c for L, _ in style_groups(synthesis)]
    offsets, off = [], 0
    for C in channels:
        offsets.append(B * off)
        off += C
    return names, channels, offsets, B * off


class StyleCodes:
    """The style codes of B images in one flat f32 leaf `flat` (what an optimiser sees; style_layout), the per-block views `blocks`
    ([B,C_g] each, on flat's storage) under `names`, and the flat gradient buffer `grads` of the same layout with its views
    `grad_blocks` - all allocated here (a captured iteration keeps the addresses).  The optimiser is the step's."""

    def __init__(self, synthesis, B, device):
        if B < 1:
            raise ValueError("StyleCodes: B must be positive")
        self.synthesis, self.B = synthesis, int(B)
        self.names, self.channels, self.offsets, self.numel = style_layout(synthesis, self.B)
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=device, requires_grad=True)
        self.grads = torch.zeros(self.numel, dtype=torch.float32, device=device)
        view = lambda t: [t[o:o + self.B * C].view(self.B, C) for o, C in zip(self.offsets, self.channels)]
        self.blocks, self.grad_blocks = view(self.flat.detach()), view(self.grads)

    def fits(self, B, device):          # whether this allocation serves a group of B images on `device`
        return self.B == B and self.flat.device == torch.device(device)

    def index(self, block):
        """The position of a block given by name (`layer3`, `output0`) or by index."""
        if isinstance(block, str):
            if block not in self.names:
                raise ValueError(f"StyleCodes: no block {block!r}; the blocks are {self.names[0]} .. {self.names[-1]}")
            return self.names.index(block)
        if not -len(self.names) <= int(block) < len(self.names):
            raise ValueError(f"StyleCodes: block index {block} outside the {len(self.names)} blocks")
        return int(block) % len(self.names)

    def set_from_wp(self, wp):
        """flat <- the styles of wp [B,L,512], in place: the one dge_linear_rows launch of synthesis(wp) (autograd_s2.styles_from_wp),
        so that synthesis(styles=self) then gives the bits of synthesis(wp).  Returns self."""
        nl, K = self.synthesis.num_layers, self.synthesis.w_space_dim
        if wp.dim() != 3 or tuple(wp.shape) != (self.B, nl, K):
            raise ValueError(f"StyleCodes.set_from_wp: wp must be {(self.B, nl, K)}, got {tuple(wp.shape)}")
        with torch.no_grad():
            styles_from_wp(self.synthesis, wp.detach(), out=self.flat.detach())
        return self

    def rows(self, b):
        """The codes of image b as the list of [1,C_g] tensors in block order: the format of `id{n}-s.pt`."""
        if not 0 <= b < self.B:
            raise ValueError(f"StyleCodes.rows: row {b} outside the {self.B} rows")
        return [blk[b:b + 1].clone() for blk in self.blocks]

    def load_rows(self, b, rows):
        """Image b's codes <- a list as `rows` returns it (or as torch.load reads `id{n}-s.pt`), in place."""
        if not 0 <= b < self.B:
            raise ValueError(f"StyleCodes.load_rows: row {b} outside the {self.B} rows")
        check_rows(rows, self.channels, "StyleCodes.load_rows")
        with torch.no_grad():
            for blk, r in zip(self.blocks, rows):
                blk[b:b + 1].copy_(r)

    def detached(self):
        """The codes as the flat tensor, detached (on flat's storage): what synthesis(styles=...) takes without a gradient."""
        return self.flat.detach()


def check_rows(rows, channels, who):
    rows = list(rows)
    if len(rows) != len(channels):
        raise ValueError(f"{who}: the codes of an image are a list of {len(channels)} tensors, got {len(rows)}")
    for g, (r, C) in enumerate(zip(rows, channels)):
        if not torch.is_tensor(r) or tuple(r.shape) != (1, C):
            raise ValueError(f"{who}: block {g} must be a tensor [1,{C}], got {tuple(r.shape) if torch.is_tensor(r) else type(r).__name__}")
    return rows


def save_style_rows(codes, rows, numbers, models_dir):
    """models_dir/id{n}-s.pt for every pair (row b, number n): StyleCodes.rows(b) on the host."""
    import os
    for b, n in zip(rows, numbers):
        torch.save([r.cpu() for r in codes.rows(b)], os.path.join(models_dir, "id%d-s.pt" % n))
