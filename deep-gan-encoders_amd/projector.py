"""StyleGAN2's projector on the HIP path (Karras et al., "Analyzing and Improving the Image Quality of StyleGAN", appendix D; the
stylegan2 / stylegan2-ada `projector.py`): the encoder-free inversion every encoder-based loop of this package is compared with
(`python -m dge_amd.compare`).  One W code [B,512], shared by all rows of W+, and the synthesis network's noise maps are optimised
with Adam (beta1 = 0.9) against LPIPS alone.  Per iteration (ProjectorStep.step):

    lr_t, noise_scale_t = projector_schedule(i, steps)                 host doubles
    ws = w + randn * noise_scale_t, in every row of W+                 dge_randn, dge_w_broadcast
    imgs = G.synthesis(ws, noises=maps)                                noise fixed to the optimised maps
    dist = LPIPS(target, imgs) per row, both area-pooled to 256^2 where the image is larger        dge_crop_pool_multi
    loss = sum_b dist_b + noise_reg * sum_b reg_b                      dge_noise_reg
    one backward: dge_area_pool_bwd, the synthesis backward with dge_s2_noise_grad, dge_w_broadcast_bwd
    one Adam step over [w, maps] with lr_t                             dge_adam_multi
    maps to zero mean and unit mean square                             dge_noise_normalize

The loss is a sum over the rows and every stage is per sample, so the B rows of a group are B independent projections; a row equals
the batch-1 run of its image.  No step makes a host synchronisation.

Decisions:
  * w_avg (also the start code) and w_std come from `w_avg_samples` z drawn from a seeded CPU generator and mapped without
    truncation, through dge_rows_mean_std; w_std = sqrt(sum (w - w_avg)^2 / samples), the projector's formula.
  * the maps start at the generator's `layer{i}.noise` buffers, a copy per row, not at fresh randn as the original does: the
    run then starts from the image G shows for w_avg, and a reloaded `id*-noise.pt` with `id*-wp.pt` reproduces `rec/*.png`.
  * the w noise of row b is a pure function of (seed, image number, iteration): the first 512 normals of dge_randn under a seed
    mixed from the three (w_noise_seed), one launch per row because the seed is the generator's key.  A captured iteration reads
    the seeds from device scalars that _graph_inputs refreshes, through dge_randn's `seed_dev`.
  * a captured iteration reads Adam's two step scalars and noise_scale from device floats (custom_adam.Adam.graph_advance,
    _graph_inputs), so the schedule moves under replay.
  * the target's VGG features are recomputed every iteration (LPIPS.value_and_grad evaluates both halves).
  * one process: WORLD_SIZE > 1 is refused.
  * ProjectorStep freezes the generator it is given (requires_grad_(False) on every parameter) and does not undo it.

Files of `project` / the CLI: real/{n:05d}.png and rec/{n:05d}.png (the bytes of infer.quantize_u8: `compare --dir1 real --dir2
rec` works on the output), models/id{n}-w.pt [1,512], models/id{n}-wp.pt [1,L,512], models/id{n}-noise.pt (the list of maps, each
[1,res,res], as embedding_v2 writes it) and Loss.txt.  Images are numbered across the folder; a short last group repeats its last
image and discards the padded rows, as `embedding_v2 --independent true` does.

Masked projection (`--mask_dir DIR|x.pt`, ProjectorStep.begin_image(mask=...), project(mask=...)): a mask [B,1,H,W] in [0,1] at the
target's size, 1 = fit the pixel, 0 = ignore it.  The mask is area-pooled with the images; both LPIPS inputs are multiplied by it
(a hole is mid-grey in both) and tap k is averaged with the weights m_k / sum m_k of the mask's level k (csrc/lpips_mask_kernels.hip,
LPIPS.value_and_grad(mask_state=...)).  The pyramid is refilled once per group, outside the captured iteration; a step captured
without a mask refuses a later mask and the other way round.  Extra files with a mask: blend/{n:05d}.png (the target inside the mask,
the reconstruction outside: the bytes of quantize_u8(ops.mask_blend(mask, real, rec))), mask/{n:05d}.png (8-bit L), and `cover: ...`
(the kept share of the image) at the end of every Loss.txt line; the result dict gains `mask_cover` [B].  A short last group pads the
mask as it pads the image.  Without a mask nothing is written or launched that was not before.

StyleSpace refinement (`--s_steps N [--s_lr x]`, StyleProjectorStep, project(styles=...)): behind the W run of a group, N iterations
that optimise the group's StyleSpace codes (style_codes.StyleCodes: the style vector of every conv layer and toRGB block, started at
the styles of the W result) and go on with its noise maps, against the same loss and under the same learning-rate ramp, without
latent noise.  rec/{n:05d}.png and id{n}-noise.pt are then those of the S stage, id{n}-w.pt and id{n}-wp.pt stay the W result,
models/id{n}-s.pt holds the codes (a list of [1,C_g] tensors; with id{n}-noise.pt it reloads into synthesis(styles=..., noises=...)
and gives the PNG byte for byte), and Loss.txt gets the stage's lines (`id_n_____s_i`).  The default --s_steps 0 changes nothing.
The base rate --s_lr defaults to 0.01; nobody has tuned that value."""
import argparse
import math
import os

import torch

from . import ops
from .custom_adam import Adam
from .embed_step import several_processes
from .graph_step import GraphReplay
from .noise_maps import NoiseMaps, save_noise_rows
from .style_codes import save_style_rows


def projector_schedule(step, steps, lr=0.1, w_std=1.0, initial_noise_factor=0.05, noise_ramp=0.75, lr_rampdown=0.25, lr_rampup=0.05):
    """(lr_t, noise_scale_t) of iteration `step` of `steps`, host doubles: the learning rate ramps up over the first `lr_rampup` of
    the run and decays by a cosine over the last `lr_rampdown`; the w noise decays quadratically to 0 at `noise_ramp`."""
    t = step / steps
    noise_scale = w_std * initial_noise_factor * max(0.0, 1.0 - t / noise_ramp) ** 2
    r = min(1.0, (1.0 - t) / lr_rampdown)
    r = 0.5 - 0.5 * math.cos(r * math.pi)
    r = r * min(1.0, t / lr_rampup)
    return lr * r, noise_scale


def w_noise_seed(seed, number, iteration):
    """The dge_randn seed of image `number`'s w noise in iteration `iteration`: splitmix64 over the three, so neighbouring
    images and iterations get unrelated Philox keys."""
    M = 0xFFFFFFFFFFFFFFFF
    x = (int(seed) * 0x9E3779B97F4A7C15 + int(number) * 0xBF58476D1CE4E5B9 + int(iteration) * 0x94D049BB133111EB + 0x2545F4914F6CDD1D) & M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
    return x ^ (x >> 31)


class _WBroadcast(torch.autograd.Function):
    """ws[b,l,:] = w[b,:] + noise[b,:] * scale (dge_w_broadcast); the gradient of w is the sum over l (dge_w_broadcast_bwd)."""

    @staticmethod
    def forward(ctx, w, noise, scale, L):
        return ops.w_broadcast(w.detach(), L, noise, scale)

    @staticmethod
    def backward(ctx, g):
        return ops.w_broadcast_bwd(g.float().contiguous()), None, None, None


class _LpipsFit(GraphReplay):
    """What the two stages of a projection share: the area pooling in front of LPIPS, the group's mask, and the per-row LPIPS value
    with the gradient of its sum w.r.t. the synthesised images."""
    POOL_TO = 256          # LPIPS runs on images of at most this side (the projector's area pooling)
    _mask_state = _mask_cover = _graph_masked = None

    def _pool_k(self, H):
        k = 1
        while H // k > self.POOL_TO:
            k *= 2
        return k

    def _set_mask(self, target, mask, who):
        """The group's mask [B,1,H,W] (or None) into the step: pooled by the step's k to the LPIPS resolution, the state refilled in
        place (one dge_mask_pyramid call outside the captured iteration), mask_cover refreshed in place."""
        cls = type(self).__name__
        if self.captured and (mask is not None) != self._graph_masked:
            raise ValueError(f"{cls}.{who}: the iteration was captured " + ("with a mask, and this group has none" if self._graph_masked
                             else "without a mask, and this group has one") + "; the masked and the unmasked iteration are different "
                             "launches: use a step of its own for each")
        if mask is None:
            self._mask_state = self._mask_cover = None
            return
        B, _, H, W = target.shape
        if mask.dim() == 3:
            mask = mask[:, None]
        if tuple(mask.shape) != (B, 1, H, W):
            raise ValueError(f"{cls}.{who}: the mask must be [B,1,H,W] = {(B, 1, H, W)} at the target's size, got {tuple(mask.shape)}")
        m = mask.detach().to(device=target.device, dtype=torch.float32).contiguous()
        k = self._pool_k(H)
        if k > 1:
            m = ops.area_pool(m, k)
        if self._mask_state is None or self._mask_state.shape != (B, m.shape[2], m.shape[3]):
            if self.captured:
                raise ValueError(f"{cls}.{who}: the captured iteration works on a different mask geometry")
            self._mask_state = self.lpips.mask_state(m)
            self._mask_cover = torch.empty(B, dtype=torch.float32, device=target.device)
        else:
            self._mask_state.set(m)
        self._mask_cover.copy_(self._mask_state.cover())

    def _dist_and_grad(self, target, imgs):
        """(dist [B], d sum_b dist_b / d imgs) of the synthesised `imgs` against `target`, both area-pooled to POOL_TO where larger,
        mask-weighted when the group has a mask."""
        B, k = target.shape[0], self._pool_k(target.shape[2])
        with torch.no_grad():
            a, b = target.float().contiguous(), imgs.detach().float().contiguous()
            if k > 1:
                a, b = ops.area_pool(a, k), ops.area_pool(b, k)
            if self._mask_state is None:
                dist, gb = self.lpips.value_and_grad(a, b, per_sample=True)
            else:
                dist, gb = self.lpips.value_and_grad(a, b, per_sample=True, mask_state=self._mask_state)
            if B > 1:
                ops.scale_(gb, B)          # value_and_grad returns d mean / d b; the loss is the sum over the rows
            return dist, (gb if k == 1 else ops.area_pool_bwd(gb, k))


class ProjectorStep(_LpipsFit):
    """One projection step (module docstring).  G is a StyleGAN2Generator in eval mode.  The constructor FREEZES G: every parameter
    gets requires_grad_(False) and keeps it (the synthesis backward then computes the data gradient only); a caller that trains
    the same G afterwards switches the flags back on itself."""
    def __init__(self, G, lpips_model, steps=1000, lr=0.1, initial_noise_factor=0.05, noise_ramp=0.75, lr_rampdown=0.25, lr_rampup=0.05,
                 noise_reg=1e5, w_avg_samples=10000, seed=0):
        if several_processes():
            raise ValueError("ProjectorStep: the projector runs in one process (WORLD_SIZE > 1 is not supported)")
        if G.training:
            raise ValueError("ProjectorStep: G must be in eval mode (G.eval()): the projection runs on fixed noise and a fixed w_avg")
        if steps < 1 or w_avg_samples < 1:
            raise ValueError("ProjectorStep: steps and w_avg_samples must be positive")
        self.G, self.lpips = G, lpips_model
        for p in G.parameters():
            p.requires_grad_(False)
        self.steps, self.lr, self.noise_reg, self.w_avg_samples, self.seed = int(steps), float(lr), float(noise_reg), int(w_avg_samples), int(seed)
        self._sched = dict(initial_noise_factor=initial_noise_factor, noise_ramp=noise_ramp, lr_rampdown=lr_rampdown, lr_rampup=lr_rampup)
        self.w_avg = self.w_std = None
        self.w = self.opt = self.noise = None          # (noise: the NoiseMaps owner, from the first group)
        self._ns_dev = self._seeds_dev = None
        self._mask_state = self._mask_cover = self._graph_masked = None
        self._inputs_fresh = False          # graph mode: _graph_inputs has uploaded the inputs of the iteration step() is about to issue
        self.group, self.it, self.numbers, self.last = -1, 0, [], {}

    # ------------------------------------------------------------------ statistics of W
    def w_stats(self, z=None, chunk=1000):
        """(w_avg [512] device tensor, w_std host float), computed once and cached on the step.  z: the samples [N,512] (parity
        runs); default: `w_avg_samples` draws of torch.randn from a CPU generator seeded with `seed`."""
        if self.w_avg is None:
            dev = next(self.G.parameters()).device
            if z is None:
                z = torch.randn(self.w_avg_samples, self.G.z_space_dim, generator=torch.Generator().manual_seed(self.seed))
            with torch.no_grad():
                ws = torch.cat([self.G.mapping(z[i:i + chunk].to(dev))["w"] for i in range(0, z.shape[0], chunk)])
                self.w_avg, std = ops.rows_mean_std(ws.float().contiguous())
            self.w_std = float(std)          # (the one host read: the schedule is a host function)
        return self.w_avg, self.w_std

    def schedule(self, iteration):
        return projector_schedule(iteration, self.steps, self.lr, self.w_stats()[1], **self._sched)

    # ------------------------------------------------------------------ per image group
    def begin_image(self, target, numbers=None, mask=None):
        """Start the group of `target` [B,3,H,W]: w = w_avg in every row, the maps = the generator's buffers in every row, Adam's
        state cleared, the iteration count at 0 - all in place (a captured iteration stays valid).  The maps are initialised from
        the generator's buffers and not from fresh randn (the original's choice): the written id*-noise.pt then reproduces the
        image with id*-wp.pt, and the run starts from the image G shows for w_avg.  numbers: the image number of every row
        (default group * B + b), which seeds its w noise.  mask [B,1,H,W] f32 in [0,1] at the target's size (1 = fit the pixel,
        0 = ignore it): the group is fitted under the mask-weighted LPIPS of LPIPS.value_and_grad(mask_state=...)."""
        B, dev = target.shape[0], target.device
        self._set_mask(target, mask, "begin_image")
        w_avg, _ = self.w_stats()
        if self.noise is None or not self.noise.fits(B, dev):          # (w is allocated with the maps: one row each per image)
            if self.captured:
                raise ValueError("ProjectorStep.begin_image: the captured iteration works on a different batch")
            D = self.G.w_space_dim
            self.w = torch.zeros((B, D), dtype=torch.float32, device=dev, requires_grad=True)
            self._wn = torch.empty((B, D), dtype=torch.float32, device=dev)
            self.noise = NoiseMaps(self.G.synthesis, B, dev)
            self.opt = Adam([self.w, self.noise.flat], lr=self.lr, betas=(0.9, 0.999), eps=1e-8)
        self.group += 1
        self.numbers = [self.group * B + b for b in range(B)] if numbers is None else [int(n) for n in numbers]
        if len(self.numbers) != B:
            raise ValueError("ProjectorStep.begin_image: one image number per row")
        with torch.no_grad():
            self.w.copy_(w_avg.reshape(1, -1).expand_as(self.w))
        self.noise.reset()
        self.opt.graph_reset()
        self.it = 0

    def _seeds(self):
        return [w_noise_seed(self.seed, n, self.it) for n in self.numbers]

    # ------------------------------------------------------------------ one iteration
    def step(self, target, w_noise=None):
        """One iteration on target [B,3,H,W] in [-1,1]; `w_noise` [B,512] replaces the draws (parity runs).  Returns w [B,512], ws
        [B,L,512] (with this iteration's noise), imgs, dist [B], reg [B], w_grad, noise_grads, noises (the maps behind the step), lr
        and noise_scale (host floats); no host synchronisation."""
        if self.group < 0:
            raise RuntimeError("ProjectorStep.step: call begin_image() first")
        graph = self._ns_dev is not None
        if graph and not self._inputs_fresh:          # an eager iteration behind capture(): it reads the device scalars too
            self._graph_inputs(self.it)
        self._inputs_fresh = False
        lr_t, ns_t = self.schedule(self.it)
        if w_noise is None:
            w_noise = ops.randn_seeded(self._wn, self._seeds(), self._seeds_dev)
        ws = _WBroadcast.apply(self.w, w_noise, self._ns_dev if graph else ns_t, self.G.num_layers)
        imgs = self.G.synthesis(ws, randomize_noise=False, noises=self.noise.maps, noise_grad_out=self.noise.grads)["image"]
        dist, g_img = self._dist_and_grad(target, imgs)
        self.w.grad = None
        imgs.backward(g_img)
        reg = self.noise.add_reg(self.noise_reg)
        self.noise.hand_grad()
        self.opt.step(lr=lr_t)
        self.noise.normalize()
        self.it += 1
        self.last = dict(w=self.w.detach(), ws=ws.detach(), imgs=imgs.detach(), dist=dist, reg=reg, w_grad=self.w.grad,
                         noise_grads=self.noise.grads, noises=self.noise.detached(), lr=lr_t, noise_scale=ns_t)
        if self._mask_state is not None:
            self.last["mask_cover"] = self._mask_cover
        return self.last

    # ------------------------------------------------------------------ hipGraph replay of the iteration
    def capture(self, target, warmup=GraphReplay.WARMUP):
        """`warmup` real iterations, then one recorded (not executed) iteration (GraphReplay._capture); begin_image() must have run
        for the group.  From here on step() reads Adam's scalars, noise_scale and the noise seeds from the device."""
        if warmup < 1:
            raise ValueError("ProjectorStep.capture: warmup must be at least 1: the first real iteration allocates Adam's state, which "
                             "a recorded iteration must find in place, and its results are what the loop reads before the first replay")
        dev = target.device
        self._graph_masked = self._mask_state is not None
        self._g_target = target.detach().clone()
        for opt, calls in self._graph_opts():
            opt.graph_begin(calls, dev)
        self._ns_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self._seeds_dev = torch.zeros(target.shape[0], dtype=torch.int64, device=dev)
        self.graph_iteration = 0

        def keep_it():          # the count of the last executed iteration (the captured one is only recorded)
            self._it_snap = self.it
        out = self._capture_keeping_last(lambda: self.step(self._g_target), warmup, after_warmup=keep_it)
        self.it = self._it_snap
        return out

    def _graph_opts(self):
        return [(self.opt, 1)]          # one Adam over [w, maps], one call per iteration

    def _graph_inputs(self, iteration):
        """What the host decides for iteration `self.it` of the group (GraphReplay's own count runs across groups), uploaded from
        fresh pageable host tensors: staged before copy_ returns, so the host may run ahead of the device."""
        lr_t, ns_t = self.schedule(self.it)
        self.opt.param_groups[0]["lr"] = lr_t
        self.opt.graph_advance()
        self._ns_dev.copy_(torch.tensor([ns_t], dtype=torch.float32))
        self._seeds_dev.copy_(torch.tensor([s - (1 << 64) if s >= (1 << 63) else s for s in self._seeds()], dtype=torch.int64))
        self._inputs_fresh = True

    def set_image(self, target, mask=None):
        """Copies a new group's images into the static input of the captured iteration (call begin_image() for the group too).
        mask: the group's mask, refilled in place into the state the captured iteration reads; None keeps what begin_image() set."""
        self._set_static("_g_target", target)
        if mask is not None:
            self._set_mask(target, mask, "set_image")

    def replay(self):
        lr_t, ns_t = self.schedule(self.it)
        out = super().replay()
        self._inputs_fresh = False
        self.it += 1
        self.last = dict(out, lr=lr_t, noise_scale=ns_t)
        return self.last

    # ------------------------------------------------------------------ the result of a group
    @torch.no_grad()
    def result(self):
        """(w [B,512], wp [B,L,512] = w in every row, maps, image): the projection as it stands, synthesised without w noise."""
        w = self.w.detach()
        wp = ops.w_broadcast(w, self.G.num_layers)
        maps = self.noise.detached()
        return w, wp, maps, self.G.synthesis(wp, randomize_noise=False, noises=maps)["image"]


class StyleProjectorStep(_LpipsFit):
    """The second stage of a projection: the StyleSpace codes of the W result (style_codes.StyleCodes: the per-channel style
    vectors of every conv layer and toRGB block) and the noise maps are refined with Adam against the same loss.  Per iteration:

        lr_t = projector_schedule(i, steps, lr)[0]                        host double; no latent noise: S has no counterpart of w_std
        imgs = G.synthesis(styles=codes, noises=maps)                     no dge_w_broadcast, no dge_linear_rows
        dist = LPIPS(target, imgs) per row, area-pooled, mask-weighted when the group has a mask     as ProjectorStep.step
        one backward ending in S form                                     dge_s2_style_grads_s, dge_s2_noise_grad
        loss += noise_reg * sum_b reg_b                                   dge_noise_reg
        one Adam step over [codes.flat, maps] with lr_t                   dge_adam_multi
        maps to zero mean and unit mean square                            dge_noise_normalize

    The loss is a sum over the rows and every stage is per sample: B rows are B independent refinements.  No step makes a host
    synchronisation.  The constructor FREEZES G as ProjectorStep does.  The base rate `lr` (--s_lr) defaults to 0.01, a value
    nobody has tuned."""

    def __init__(self, G, lpips_model, steps=100, lr=0.01, lr_rampdown=0.25, lr_rampup=0.05, noise_reg=1e5):
        if several_processes():
            raise ValueError("StyleProjectorStep: the projector runs in one process (WORLD_SIZE > 1 is not supported)")
        if G.training:
            raise ValueError("StyleProjectorStep: G must be in eval mode (G.eval()): the refinement runs on fixed noise maps")
        if steps < 1:
            raise ValueError("StyleProjectorStep: steps must be positive")
        self.G, self.lpips = G, lpips_model
        for p in G.parameters():
            p.requires_grad_(False)
        self.steps, self.lr, self.noise_reg = int(steps), float(lr), float(noise_reg)
        self._sched = dict(lr_rampdown=lr_rampdown, lr_rampup=lr_rampup)
        self.codes = self.noise = self.opt = None
        self._graph_mode = self._inputs_fresh = False
        self.group, self.it, self.numbers, self.last = -1, 0, [], {}

    def schedule(self, iteration):
        """lr of iteration `iteration`: projector_schedule's ramp on the base rate."""
        return projector_schedule(iteration, self.steps, self.lr, **self._sched)[0]

    # ------------------------------------------------------------------ per image group
    def begin_image(self, target, wp, noises=None, numbers=None, mask=None):
        """Start the group of `target` [B,3,H,W] from the W stage's result: the codes = the styles of wp [B,L,512] (one
        dge_linear_rows launch: synthesis(styles=codes) starts at the bits of synthesis(wp)); the maps = `noises` - a NoiseMaps
        (the W stage's own: the stage goes on with it, in place), a list of maps [B,res,res] (copied), or None: the generator's
        buffers in every row; Adam's state cleared, the count at 0 - all in place (a captured iteration stays valid)."""
        B, dev = target.shape[0], target.device
        self._set_mask(target, mask, "begin_image")
        shared = noises if isinstance(noises, NoiseMaps) else None
        if shared is not None and not shared.fits(B, dev):
            raise ValueError("StyleProjectorStep.begin_image: the NoiseMaps given holds another batch than the target")
        fresh = self.codes is None or not self.codes.fits(B, dev) or (shared is not None and shared is not self.noise)
        if fresh:
            if self.captured:
                raise ValueError("StyleProjectorStep.begin_image: the captured iteration works on a different batch or on other noise maps")
            from .style_codes import StyleCodes
            self.codes = StyleCodes(self.G.synthesis, B, dev)
            self.noise = shared if shared is not None else NoiseMaps(self.G.synthesis, B, dev)
            self._own_noise = shared is None
            self.opt = Adam([self.codes.flat, self.noise.flat], lr=self.lr, betas=(0.9, 0.999), eps=1e-8)
        elif shared is None and not self._own_noise:
            raise ValueError("StyleProjectorStep.begin_image: this step runs on a shared NoiseMaps; pass it again")
        self.group += 1
        self.numbers = [self.group * B + b for b in range(B)] if numbers is None else [int(n) for n in numbers]
        if len(self.numbers) != B:
            raise ValueError("StyleProjectorStep.begin_image: one image number per row")
        self.codes.set_from_wp(wp)
        if shared is None:
            if noises is None:
                self.noise.reset()
            else:
                from .autograd_s2 import check_noises
                with torch.no_grad():
                    for m, n in zip(self.noise.maps, check_noises(self.G.synthesis, [n.detach() for n in noises], B, dev)):
                        m.copy_(n.expand_as(m))
        self.opt.graph_reset()
        self.it = 0

    # ------------------------------------------------------------------ one iteration
    def step(self, target):
        """One iteration on target [B,3,H,W] in [-1,1].  Returns styles (the flat codes behind the step), imgs, dist [B], reg [B],
        style_grad (flat), noise_grads, noises, lr; no host synchronisation."""
        if self.group < 0:
            raise RuntimeError("StyleProjectorStep.step: call begin_image() first")
        if self._graph_mode and not self._inputs_fresh:          # an eager iteration behind capture(): it reads the device scalars too
            self._graph_inputs(self.it)
        self._inputs_fresh = False
        lr_t = self.schedule(self.it)
        imgs = self.G.synthesis(styles=self.codes, randomize_noise=False, noises=self.noise.maps, noise_grad_out=self.noise.grads,
                                style_grad_out=self.codes.grads)["image"]
        dist, g_img = self._dist_and_grad(target, imgs)
        imgs.backward(g_img)
        reg = self.noise.add_reg(self.noise_reg)
        self.codes.flat.grad = self.codes.grads
        self.noise.hand_grad()
        self.opt.step(lr=lr_t)
        self.noise.normalize()
        self.it += 1
        self.last = dict(styles=self.codes.detached(), imgs=imgs.detach(), dist=dist, reg=reg, style_grad=self.codes.grads,
                         noise_grads=self.noise.grads, noises=self.noise.detached(), lr=lr_t)
        if self._mask_state is not None:
            self.last["mask_cover"] = self._mask_cover
        return self.last

    # ------------------------------------------------------------------ hipGraph replay of the iteration
    def capture(self, target, warmup=GraphReplay.WARMUP):
        """`warmup` real iterations, then one recorded (not executed) iteration (GraphReplay._capture); begin_image() must have run
        for the group.  From here on step() reads Adam's scalars from the device."""
        if warmup < 1:
            raise ValueError("StyleProjectorStep.capture: warmup must be at least 1: the first real iteration allocates Adam's state, "
                             "which a recorded iteration must find in place, and its results are what the loop reads before the first replay")
        self._graph_masked = self._mask_state is not None
        self._g_target = target.detach().clone()
        for opt, calls in self._graph_opts():
            opt.graph_begin(calls, target.device)
        self._graph_mode = True
        self.graph_iteration = 0

        def keep_it():          # the count of the last executed iteration (the captured one is only recorded)
            self._it_snap = self.it
        out = self._capture_keeping_last(lambda: self.step(self._g_target), warmup, after_warmup=keep_it)
        self.it = self._it_snap
        return out

    def _graph_opts(self):
        return [(self.opt, 1)]          # one Adam over [codes, maps], one call per iteration

    def _graph_inputs(self, iteration):
        """The learning rate of iteration `self.it` of the group into Adam's device scalars (GraphReplay's own count runs across groups)."""
        self.opt.param_groups[0]["lr"] = self.schedule(self.it)
        self.opt.graph_advance()
        self._inputs_fresh = True

    def set_image(self, target, mask=None):
        """Copies a new group's images into the static input of the captured iteration (call begin_image() for the group too)."""
        self._set_static("_g_target", target)
        if mask is not None:
            self._set_mask(target, mask, "set_image")

    def replay(self):
        lr_t = self.schedule(self.it)
        out = super().replay()
        self._inputs_fresh = False
        self.it += 1
        self.last = dict(out, lr=lr_t)
        return self.last

    # ------------------------------------------------------------------ the result of a group
    @torch.no_grad()
    def result(self):
        """(codes: the StyleCodes, maps, image): the refinement as it stands."""
        maps = self.noise.detached()
        return self.codes, maps, self.G.synthesis(styles=self.codes.detached(), randomize_noise=False, noises=maps)["image"]


def project(st, target, out_dir=None, save_every=100, launch="graph", numbers=None, keep=None, mask=None, styles=None):
    """`st.steps` iterations on the group `target` [B,3,H,W]; launch="graph" captures the iteration once (its warm-up iteration is a
    real one) and replays it, later groups go through set_image.  With `out_dir`: a Loss.txt line per kept row at every
    `save_every`-th iteration and at the end (one host read each), and the files of the module docstring for the first `keep` rows
    (default: all), numbered by `numbers`.  Returns the last result dict with `w`, `wp`, `noises` and `rec` of ProjectorStep.result().
    mask [B,1,H,W] f32 in [0,1] at the target's size: the masked projection (ProjectorStep.begin_image); the Loss.txt lines then end
    in `cover: ...`, and blend/{n:05d}.png (the target where the mask is 1, the reconstruction where it is 0:
    quantize_u8(ops.mask_blend(mask, real, rec))) and mask/{n:05d}.png (8-bit L) are written next to real/ and rec/.
    styles: a StyleProjectorStep - behind the W run its `steps` iterations refine the group in StyleSpace, from this group's wp and
    on its maps (in place, the W step's NoiseMaps); rec/, blend/ and id{n}-noise.pt are then those of the S stage, id{n}-w.pt and
    id{n}-wp.pt stay the W result, models/id{n}-s.pt (StyleCodes.rows) is written, Loss.txt gets the stage's lines (`id_n_____s_i`),
    and the result dict carries the S stage's `dist` / `reg` and `styles` (the StyleCodes)."""
    from .embedding import iterate
    from .infer import quantize_u8, save_u8
    iterations = iterate(st, target, st.steps, launch)          # (validates `launch` here; starts behind begin_image, in the loop)
    B = target.shape[0]
    keep = B if keep is None else keep
    if mask is None:
        st.begin_image(target, numbers=numbers)
    else:
        if mask.dim() == 3:
            mask = mask[:, None]
        mask = mask.to(device=target.device, dtype=torch.float32).contiguous()
        st.begin_image(target, numbers=numbers, mask=mask)
    nums = st.numbers

    def log(i, r, stage="i"):
        vals = torch.stack((r["dist"], r["reg"]) + ((r["mask_cover"],) if mask is not None else ())).cpu()
        with open(os.path.join(out_dir, "Loss.txt"), "a+") as f:
            for b in range(keep):
                line = "id_%d_____%s_%d  dist: %s  noise_reg: %s  lr: %s  noise_scale: %s" % (nums[b], stage, i, float(vals[0, b]),
                                                                                         float(vals[1, b]), r["lr"], r["noise_scale"])
                print(line if mask is None else line + "  cover: %s" % float(vals[2, b]), file=f)
    for i, r in iterations:          # (st.steps >= 1: the loop runs and leaves the last result in r)
        if out_dir is not None and save_every and (i % save_every == 0 or i == st.steps - 1):
            log(i, r)
    w, wp, maps, rec = st.result()
    codes = None
    if styles is not None:
        s_iterations = iterate(styles, target, styles.steps, launch)
        styles.begin_image(target, wp, noises=st.noise, numbers=nums, mask=mask)
        for i, rs in s_iterations:
            if out_dir is not None and save_every and (i % save_every == 0 or i == styles.steps - 1):
                log(i, dict(rs, noise_scale=0.0), "s")
        codes, maps, rec = styles.result()
        r = dict(r, dist=rs["dist"], reg=rs["reg"], styles=codes)
    if out_dir is not None:
        for sub in ("real", "rec", "models") + (("blend", "mask") if mask is not None else ()):
            os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
        q_real, q_rec = quantize_u8(target.float()), quantize_u8(rec)
        if mask is not None:
            q_blend = quantize_u8(ops.mask_blend(mask, target.float().contiguous(), rec.float().contiguous()))
            q_mask = mask_u8(mask)
        wc, wpc, mc = w.cpu(), wp.cpu(), [m.cpu() for m in maps]
        for b in range(keep):
            n = nums[b]
            save_u8(q_real[b], os.path.join(out_dir, "real", "%05d.png" % n))
            save_u8(q_rec[b], os.path.join(out_dir, "rec", "%05d.png" % n))
            if mask is not None:
                save_u8(q_blend[b], os.path.join(out_dir, "blend", "%05d.png" % n))
                save_u8(q_mask[b], os.path.join(out_dir, "mask", "%05d.png" % n))
            torch.save(wc[b:b + 1].clone(), os.path.join(out_dir, "models", "id%d-w.pt" % n))
            torch.save(wpc[b:b + 1].clone(), os.path.join(out_dir, "models", "id%d-wp.pt" % n))
        save_noise_rows(mc, range(keep), nums[:keep], os.path.join(out_dir, "models"))
        if codes is not None:
            save_style_rows(codes, range(keep), nums[:keep], os.path.join(out_dir, "models"))
    return dict(r, w=w, wp=wp, noises=maps, rec=rec)


def mask_u8(mask):
    """mask [B,1,H,W] in [0,1] -> [B,H,W] uint8 on the host, round(255 m): what mask/{n:05d}.png holds (a mask read from an 8-bit
    file comes back with its bytes)."""
    return (mask.detach().float().cpu()[:, 0] * 255.0).round().clamp(0, 255).to(torch.uint8)


def load_masks(path, size, n_images):
    """--mask_dir: a folder (files in sorted-name order pair with the images of --img_dir in theirs; decoded as 8-bit L, resized
    to size x size with PIL's bilinear filter, / 255: white = fit) or a .pt tensor [N,1,H,W] or [N,H,W] in [0,1] -> [N,1,size,size]
    f32 on the host.  Exits when the count differs from the images'."""
    if path.endswith(".pt"):
        m = torch.load(path, map_location="cpu").float()
        if m.dim() == 3:
            m = m[:, None]
        if m.dim() != 4 or m.shape[1] != 1:
            raise SystemExit(f"projector: --mask_dir {path}: expected [N,1,H,W] or [N,H,W], got {tuple(m.shape)}")
        if tuple(m.shape[2:]) != (size, size):
            raise SystemExit(f"projector: --mask_dir {path}: the masks are {tuple(m.shape[2:])}, the images {(size, size)}")
        if float(m.min()) < 0.0 or float(m.max()) > 1.0:
            raise SystemExit(f"projector: --mask_dir {path}: values outside [0,1]")
    else:
        import numpy as np
        from PIL import Image
        from .embedding_v2 import IMAGE_EXT
        names = sorted(n for n in os.listdir(path) if n.lower().endswith(IMAGE_EXT))
        planes = [torch.from_numpy(np.asarray(Image.open(os.path.join(path, n)).convert("L").resize((size, size), Image.BILINEAR),
                                              dtype=np.uint8).copy()).float().div(255.0) for n in names]
        m = torch.stack(planes)[:, None] if planes else torch.zeros((0, 1, size, size))
    if m.shape[0] != n_images:
        raise SystemExit(f"projector: --mask_dir {path} holds {m.shape[0]} masks, --img_dir {n_images} images: one mask per image")
    return m.contiguous()


# ------------------------------------------------------------------ CLI
def make_parser():
    from .embedding_v2 import strict_bool
    from .infer import add_lpips_args
    from .models import add_model_args
    p = argparse.ArgumentParser(prog="dge_amd.projector", description="StyleGAN2's projector: W and noise-map optimisation against LPIPS")
    add_model_args(p)
    p.set_defaults(mtype=2)
    p.add_argument("--img_dir", default="./real_imgs/", help="a directory of images or a .pt tensor in [0,1]")
    p.add_argument("--mask_dir", default=None, help="masks, one per image: a directory (sorted-name order, white = fit) or a .pt "
                   "tensor [N,1,H,W] / [N,H,W] in [0,1]; the projection then fits the masked region only")
    p.add_argument("--experiment_dir", default="./projector_result")
    p.add_argument("--steps", type=int, default=1000)
    p.add_argument("--batch_size", type=int, default=1, help="images projected side by side, each as in its batch-1 run")
    p.add_argument("--lr", type=float, default=0.1)
    p.add_argument("--initial_noise_factor", type=float, default=0.05)
    p.add_argument("--noise_ramp", type=float, default=0.75)
    p.add_argument("--lr_rampdown", type=float, default=0.25)
    p.add_argument("--lr_rampup", type=float, default=0.05)
    p.add_argument("--noise_reg", type=float, default=1e5, help="weight of the noise regulariser")
    p.add_argument("--w_avg_samples", type=int, default=10000)
    p.add_argument("--s_steps", type=int, default=0, help="iterations of the StyleSpace refinement behind every W run (0: none): the "
                   "style codes of the W result and the noise maps are optimised further; writes models/id{n}-s.pt")
    p.add_argument("--s_lr", type=float, default=0.01, help="base learning rate of the StyleSpace refinement (an untuned default)")
    p.add_argument("--launch", choices=("eager", "graph"), default="graph")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--save_every", type=int, default=100)
    p.add_argument("--deterministic", type=strict_bool, default=False, help="true: bit-reproducible reductions (ops.set_deterministic)")
    add_lpips_args(p)
    return p


def parse_args(argv=None):
    args = make_parser().parse_args(argv)
    if args.mtype != 2:
        raise SystemExit("projector: --mtype must be 2 (StyleGAN2): StyleGAN1, PGGAN and BigGAN are not offered")
    if several_processes(env=True):
        raise SystemExit("projector: runs in one process (WORLD_SIZE > 1 is not supported)")
    if args.steps < 1 or args.batch_size < 1:
        raise SystemExit("projector: --steps and --batch_size must be positive")
    if args.s_steps < 0:
        raise SystemExit("projector: --s_steps must be 0 (no StyleSpace refinement) or positive")
    if args.s_steps and not args.s_lr > 0.0:
        raise SystemExit("projector: --s_lr must be positive")
    return args


def main(argv=None):
    from .embedding_v2 import _load_imgs, load_generator_smooth, rows_plan
    from .lpips import LPIPS
    from .models import load_lpips_weights
    from .stylegan2_generator import StyleGAN2Generator
    args = parse_args(argv)
    if args.deterministic:
        ops.set_deterministic(True)
    dev = "cuda"
    torch.manual_seed(args.seed)
    kw = {k: getattr(args, k) for k in ("fmaps_base", "fmaps_max") if getattr(args, k) is not None}
    G = StyleGAN2Generator(args.img_size, compute_dtype=args.compute_dtype, **kw).to(dev)
    G.eval()
    if args.checkpoint_dir_GAN:
        load_generator_smooth(G, args.checkpoint_dir_GAN)
    LP = load_lpips_weights(LPIPS(compute_dtype=args.compute_dtype).to(dev), args.vgg_weights, args.lpips_weights,
                            allow_standin=args.allow_standin_lpips)
    out = args.experiment_dir
    os.makedirs(out, exist_ok=True)
    imgs = _load_imgs(args.img_dir, args.img_size, dev)
    masks = load_masks(args.mask_dir, args.img_size, imgs.shape[0]).to(dev) if args.mask_dir else None
    st = ProjectorStep(G, LP, steps=args.steps, lr=args.lr, initial_noise_factor=args.initial_noise_factor, noise_ramp=args.noise_ramp,
                       lr_rampdown=args.lr_rampdown, lr_rampup=args.lr_rampup, noise_reg=args.noise_reg, w_avg_samples=args.w_avg_samples,
                       seed=args.seed)
    sst = StyleProjectorStep(G, LP, steps=args.s_steps, lr=args.s_lr, lr_rampdown=args.lr_rampdown, lr_rampup=args.lr_rampup,
                             noise_reg=args.noise_reg) if args.s_steps else None
    for first, keep, idx, _ in rows_plan(imgs.shape[0], args.batch_size):
        r = project(st, imgs[idx].contiguous(), out, args.save_every, args.launch, numbers=idx, keep=keep,
                    mask=None if masks is None else masks[idx].contiguous(), styles=sst)
        vals = torch.stack((r["dist"], r["reg"])).cpu()
        for b in range(keep):
            print("image %d: dist %.5f  noise_reg %.3e" % (first + b, float(vals[0, b]), float(vals[1, b])))
    st.style_stage = sst          # (the StyleProjectorStep of --s_steps, or None)
    return st


if __name__ == "__main__":
    main()
