"""PGGAN generator (reference model/pggan/pggan_generator.py: PGGANGenerator :28-204,
ConvBlock :236-339) on the HIP kernels.  Same constructor arguments, forward signature, result
dict and state_dict keys (`lod`, `layer{i}.{weight,bias}`, `output{k}.{weight,bias}`; 43 keys at
256).  Per block: pixel norm -> [nearest x2] -> conv (weight*sqrt(2)/sqrt(fan_in)) + bias ->
lrelu(0.2); `layer0` is the 4x4 "dense" conv on the 1x1 latent.  The nearest upsample is fused
into the conv read, bias + activation into its epilogue.  Only lod == 0 (what the released
checkpoints and E_align use) is implemented; the stray `print(x.shape)` of the reference (:196) is
not reproduced.
"""
import numpy as np
import torch
from torch import nn

from . import ops
from .stylegan2_generator import _dt
from .weight_cache import lookup, store

_RESOLUTIONS_ALLOWED = [8, 16, 32, 64, 128, 256, 512, 1024]
_INIT_RES = 4


class ConvBlock(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=3, padding=1, upsample=False, wscale_gain=np.sqrt(2.0),
                 activation_type="lrelu"):
        super().__init__()
        self.in_c, self.out_c, self.ksize, self.padding, self.upsample = in_channels, out_channels, kernel_size, padding, upsample
        self.weight = nn.Parameter(torch.randn(out_channels, in_channels, kernel_size, kernel_size))
        self.wscale = wscale_gain / np.sqrt(kernel_size * kernel_size * in_channels)
        self.bias = nn.Parameter(torch.zeros(out_channels))
        if activation_type not in ("linear", "lrelu"):
            raise NotImplementedError(f"Not implemented activation function: `{activation_type}`!")
        self.act = ops.ACT_LRELU if activation_type == "lrelu" else ops.ACT_NONE
        self._cache = {}

    def packed(self, dtype, mode=ops.PACK_FWD):
        key = (mode, dtype)
        hit = lookup(self._cache, key, self.weight)
        if hit is None:
            hit = store(self._cache, key, self.weight, ops.pack_conv_weight(self.weight, mode, dtype, self.wscale))
        return hit


class PGGANGenerator(nn.Module):
    def __init__(self, resolution, z_space_dim=512, image_channels=3, final_tanh=False, label_size=0, fused_scale=False,
                 use_wscale=True, fmaps_base=16 << 10, fmaps_max=512, compute_dtype="bf16"):
        super().__init__()
        if resolution not in _RESOLUTIONS_ALLOWED:
            raise ValueError(f"Invalid resolution: `{resolution}`!\nResolutions allowed: {_RESOLUTIONS_ALLOWED}.")
        if image_channels != 3 or final_tanh or label_size or fused_scale or not use_wscale:
            raise ValueError("only the released-checkpoint configuration is implemented (3 channels, no tanh, no labels, "
                             "fused_scale=False, use_wscale=True)")
        _dt(compute_dtype)
        self.compute_dtype = compute_dtype
        self.init_res, self.resolution, self.z_space_dim = _INIT_RES, resolution, z_space_dim
        self.init_res_log2, self.final_res_log2 = 2, int(np.log2(resolution))
        self.fmaps_base, self.fmaps_max = fmaps_base, fmaps_max
        self.num_layers = (self.final_res_log2 - self.init_res_log2 + 1) * 2
        self.register_buffer("lod", torch.zeros(()))
        for res_log2 in range(self.init_res_log2, self.final_res_log2 + 1):
            res = 2 ** res_log2
            k = res_log2 - self.init_res_log2
            if res == self.init_res:
                self.add_module(f"layer{2 * k}", ConvBlock(z_space_dim, self.get_nf(res), kernel_size=4, padding=3))
            else:
                self.add_module(f"layer{2 * k}", ConvBlock(self.get_nf(res // 2), self.get_nf(res), upsample=True))
            self.add_module(f"layer{2 * k + 1}", ConvBlock(self.get_nf(res), self.get_nf(res)))
            self.add_module(f"output{k}", ConvBlock(self.get_nf(res), image_channels, kernel_size=1, padding=0,
                                                    wscale_gain=1.0, activation_type="linear"))

    def get_nf(self, res):
        return min(self.fmaps_base // res, self.fmaps_max)

    def _dense0_weight(self):
        """layer0 is conv2d(4x4, pad 3) on a 1x1 input == a dense layer: out[(y,x),o] = sum_c z_c W[o,c,3-y,3-x]."""
        L = self.layer0
        hit = lookup(L._cache, "dense0", L.weight)
        if hit is None:
            w = L.weight.detach().flip(2, 3).permute(2, 3, 0, 1).reshape(16 * L.out_c, L.in_c).contiguous()
            hit = store(L._cache, "dense0", L.weight, (w, L.bias.detach().repeat(16).contiguous()))
        return hit

    def forward(self, z, label=None, lod=None, fused_backward=False, **_unused_kwargs):
        """fused_backward: the backward runs every pixel-norm backward -> activation backward pair (with the nearest-upsample adjoint
        of an up layer in between) as one ops.pixelnorm_act_bwd launch; the forward and the default backward are unchanged."""
        if z.ndim != 2 or z.shape[1] != self.z_space_dim:
            raise ValueError(f"Input latent code should be with shape [batch_size, latent_dim], where `latent_dim` equals "
                             f"to {self.z_space_dim}!\nBut `{z.shape}` is received!")
        lod = float(self.lod) if lod is None else lod
        if lod != 0:
            raise ValueError("only lod == 0 is implemented (the released generators are fully grown)")
        image, zn = _PGGANFunction.apply(self, z, bool(fused_backward))
        return {"z": zn, "label": label, "image": image}

    # ------------------------------------------------------------------ pipelines
    def _run(self, z, save):
        dt = _dt(self.compute_dtype)
        B = z.shape[0]
        zf = z.float().contiguous()
        zn = ops.pixelnorm(zf)
        wd, bd = self._dense0_weight()
        h = ops.linear(zn, wd, bd, wscale=self.layer0.wscale, act=ops.ACT_LRELU)           # [B, 16*C0] == NHWC [B,4,4,C0]
        C0 = self.layer0.out_c
        x = ops.nchw_to_nhwc(h.view(B, 16 * C0, 1, 1), B, dt).view(B, 4, 4, C0)
        saved = dict(z=zf, h=h, convs=[]) if save else None
        nblk = self.final_res_log2 - self.init_res_log2 + 1
        for k in range(nblk):
            if k > 0:
                L = getattr(self, f"layer{2 * k}")
                y = ops.conv2d(ops.pixelnorm_nhwc(x), L.packed(dt), L.out_c, 3, bias=L.bias.detach(), act=L.act, in_up2=True)
                if save:
                    saved["convs"].append((L, x, y, True))
                x = y
            L = getattr(self, f"layer{2 * k + 1}")
            y = ops.conv2d(ops.pixelnorm_nhwc(x), L.packed(dt), L.out_c, 3, bias=L.bias.detach(), act=L.act)
            if save:
                saved["convs"].append((L, x, y, False))
            x = y
        O_ = getattr(self, f"output{nblk - 1}")
        ones = torch.ones((B, x.shape[3]), dtype=torch.float32, device=x.device)
        xn = ops.pixelnorm_nhwc(x)
        image = ops.torgb(xn, O_.weight.detach().reshape(3, -1), ones, O_.bias.detach(), None, O_.wscale)
        if save:
            saved.update(x_last=x, xn_last=xn, out=O_)
        return image, zn, saved

    def _backward(self, saved, g_image, fused=False):
        """d(image)/d(z) contracted with g_image (hand-written data gradient; the generator's parameters are frozen in E_align).
        `fused`: between two data-gradient convs (and behind torgb_bwd) one ops.pixelnorm_act_bwd launch stands for
        [nearest_up2_bwd ->] pixelnorm_nhwc_bwd -> act_bwd: the activation the pixel norm read is the previous conv's leaky-relu
        output, so both factors come from one read of it and the gradient is not rounded in between.  A channel count the launch
        refuses takes the composed launches; the dense layer-0 tail is the same in both forms."""
        dt = ops.dtype_of(saved["x_last"])
        B = g_image.shape[0]
        O_ = saved["out"]
        ones = torch.ones((B, saved["x_last"].shape[3]), dtype=torch.float32, device=g_image.device)
        g_xn, _ = ops.torgb_bwd(g_image.float().contiguous(), saved["xn_last"], O_.weight.detach().reshape(3, -1), ones, O_.wscale)
        convs = saved["convs"]

        def fuse(i):
            """whether the pixel norm in front of convs[i + 1] (i == len - 1: in front of the output layer) is fused with the
            activation backward of convs[i], whose output it read"""
            return fused and convs[i][0].act == ops.ACT_LRELU and ops.pixelnorm_act_bwd_supported(convs[i][2].shape[3], dt)
        last = len(convs) - 1
        if fuse(last):
            g, pre_done = ops.pixelnorm_act_bwd(g_xn, saved["x_last"]), True
        else:
            g, pre_done = ops.pixelnorm_nhwc_bwd(g_xn, saved["x_last"]), False
        for i in range(last, -1, -1):
            L, x_in, y, up = convs[i]
            g_pre = g if pre_done or L.act != ops.ACT_LRELU else ops.act_bwd(g, y, None, pool=False, scale=1.0)
            g_xn = ops.conv2d(g_pre, L.packed(dt, ops.PACK_DGRAD), L.in_c, 3)
            if i > 0 and fuse(i - 1):                       # x_in is convs[i - 1]'s output
                g, pre_done = ops.pixelnorm_act_bwd(g_xn, x_in, up=up), True
                continue
            if up:
                g_xn, _ = ops.nearest_up2_bwd(g_xn)
            g, pre_done = ops.pixelnorm_nhwc_bwd(g_xn, x_in), False
        # layer0: h = lrelu(wscale * zn @ wd^T + bd) viewed as NHWC [B,4,4,C0]
        C0 = self.layer0.out_c
        g_h = ops.nhwc_to_nchw(g.view(B, 1, 1, 16 * C0)).view(B, 4, 4, C0)          # f32, same (y, x, c) order as h
        g_hpre = ops.act_bwd(g_h, saved["h"].view(B, 4, 4, C0), None, pool=False, scale=1.0).view(B, 16 * C0)
        wd, _ = self._dense0_weight()
        g_zn = torch.empty((B, self.z_space_dim), dtype=torch.float32, device=g_image.device)
        ops.linear_t(g_hpre, wd, g_zn, scale=self.layer0.wscale)
        return ops.pixelnorm_nhwc_bwd(g_zn.view(B, 1, 1, -1), saved["z"].view(B, 1, 1, -1)).view(B, -1)


class _PGGANFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, G, z, fused_backward=False):
        need = ctx.needs_input_grad[1]
        image, zn, saved = G._run(z.detach(), save=need)
        ctx.G, ctx.saved_acts, ctx.fused = G, saved, fused_backward
        ctx.mark_non_differentiable(zn)
        return image, zn

    @staticmethod
    def backward(ctx, g_image, _g_zn):
        if ctx.saved_acts is None:
            raise RuntimeError("PGGAN forward ran without saved activations")
        return None, ctx.G._backward(ctx.saved_acts, g_image, ctx.fused), None
