"""Real-image inversion of the reference's v2 scripts (embedding_v2_styleGAN1.py:71-189, embedding_v2_styleGAN2.py:82-210) on the
HIP path, for StyleGAN1 (`--mtype 1`: Gs + E_Blur) and StyleGAN2 (`--mtype 2`: StyleGAN2 synthesis + E_Blur), in two modes
(`--encoder be` puts E.BE, the encoder E_align trains, in E_Blur's place):

  mode "E" (--optimizeE true):  the encoder is re-loaded per image group and fine-tuned; w1 = E(imgs1) every iteration.
  mode "W" (--optimizeE false): the encoder is frozen and the W+ code w1 itself is optimised (LREQAdam on the leaf w1).
  mode "Z" (--optimizeE false --space z): the encoder is frozen and z [B, 512] in front of the mapping network is optimised.

Per iteration (both generators):

    [E] const2, w1 = E(imgs1);   imgs2 = G(w1)
    loss_msiv = L(img) + 0.375*L(medium) + 0.625*L(small)       (all three windows carry gradient: v2 drops the .detach())
    zero_grad; loss_msiv.backward(retain_graph=True); step
    const3, w2 = E(imgs2)                                       (StyleGAN1: right after G, before the step above; StyleGAN2: here)
    loss_msLv = 0.01*(space_loss(w1, w2) + space_loss(const2, const3)) + beta*||w1||_p;  zero_grad; backward; step

||w1||_p is Tensor.norm(p) over the whole tensor (every row of the batch).  Phase 2 back-propagates through the synthesis graph of
this iteration (its activations from before the phase-1 update), its direct terms see the updated w1: the reference's `p.data`
Adam update.

Decisions where the reference cannot run as written:
  * W mode, StyleGAN1: const2 comes from the single E(imgs1) that initialises w1; its graph would be freed by the first phase-2
    backward (the reference fails in iteration 2), so const2 is a constant.  const3's path E -> imgs2 -> G -> w1 stays live.
  * W mode, StyleGAN2: const2 is never defined in the reference (NameError): the space_loss(const2, const3) term is dropped;
    the unused loss_c2 of v1 is left out.
  * StyleGAN2 generator: the script's wrapper (truncation=0.7, use_w=True) is not in the reference tree.  It is read as a
    rosinality-style wrapper: truncation avg + psi*(w1 - avg) on every row of the W+ code, noise fixed (randomize_noise=False),
    output in [-1, 1].  psi is `truncation` (1: the plain synthesis(w1)).
  * Trackers are device-side (embed_track.EmbedTracker, dge_embed_track): the device keeps the latest best latent of each kind and
    a bounded event log (iteration, kind, loss, norm); the host writes the final best .pt per kind with the reference's file
    names and loss_min.txt from the log at the end of each group (finish_group).
  * W mode takes a batch B >= 1 (the reference hard-codes 1); the norm and space_loss terms couple the rows as in the reference.
    StyleGAN2's W-mode start is randn(B, L, 512) from a seeded generator (unseeded in the reference).
  * --optimizeE parses true / false strictly (the reference's `type=bool` cannot be switched off).
  * `independent` (--independent true; W mode, and Z mode below): the B rows of a group are B inversions of their own, each equal to the
    batch-1 run of its image.  Every loss and logged value of row b is what the coupled code returns on the one-row slices
    (losses.image_loss_tsa_rows / space_loss_rows, ||w1[b]||_p); phase 1 back-propagates sum_b loss_msiv_b, phase 2
    sum_b (0.01*lat_b + beta*||w1[b]||_p), so row b of w1.grad is the gradient of row b's own loss and Adam (element-wise) gives
    the row the steps it would take alone.  Decisions of this mode:
      - one tracker per row (iteration counter, minima, event ring, best latents); the minima of EVERY row restart at
        begin_image for both generators: the StyleGAN2 carry-over between groups is a property of the sequential batch-1 loop
        (image k inherits image k-1's minima) and has no counterpart among rows that run side by side - it stays there;
      - StyleGAN2 start code: row b of group g draws randn(1, L, 512) from manual_seed(seed + g*B + b), the draw a batch-1 run
        makes for image number g*B + b;
      - files are numbered by image (g*B + b), not by group; main() pads a short last group by repeating its last image (the
        captured iteration keeps its shape) and discards the padded rows' outputs;
      - the encoder is shared by a group, so mode "E" has no independent form (ValueError).

Generator kind "pg" (embedding_v2_pggan.PGEmbedStep: PGGAN + E_PG) runs the same iteration on z [B, z_space_dim] through three
hooks - _latent_shape, _encode (E_PG has no const output: const2 / const3 / loss_c1 are None) and _generate - in StyleGAN1's
order and with its defaults and tracker rules; "sg1" and "sg2" issue the launches they issued before.

Mode "Z" (StyleGAN1 and StyleGAN2; the baseline every W+ result is compared against, and the only code that stays on the
generator's sampling distribution).  The reference has no v2 Z-space script (its Z-space baseline is
baseline_utils/image2stylegan_w2z_opW.py): this is the v2 loop with the latent moved in front of the mapping network, as
embedding_v2_pggan is for PGGAN.  Per iteration:

    wp = trunc(map(z));  imgs2 = G(wp)
    phase 1 as above (zero_grad; loss_msiv.backward(retain_graph=True); step on z)
    w2 = E(imgs2) at the point the generator kind evaluates it above
    wp' = trunc(map(z)) from the updated z (nine small launches): the Z-mode counterpart of W mode's in-place leaf
    loss_msLv = 0.01*(space_loss(wp', w2) [+ space_loss(const2, const3), StyleGAN1]) + beta*||z||_p;  zero_grad; backward; step

  * the norm penalty is on z (the optimised leaf, as ||w1||_p is in W mode); the encoder stays the frozen W+ regulariser: it is
    compared with wp', never with z.
  * StyleGAN2: psi = `truncation` (default 0.7) on every row of wp - the reading of the wrapper W mode uses; 1 skips it.
    StyleGAN1: Gm(z, coefs) with the scripts' coefficients (0.7 on the first half of the rows) when Gm carries the truncation
    centre (center_tensor.pt), the plain broadcast otherwise; const2 = E(imgs1)'s const output, a constant as in W mode.
  * start code: `w_init` taken as z, else seeded randn with W mode's StyleGAN2 seeds (seed + group; seed + g*B + b per row).
  * the mapping adjoint runs three times per iteration: in phase 1, and in phase 2 through the old graph (w2 -> imgs2 -> wp) and
    through wp'.  The pixel-norm adjoint of the old graph reads the updated z (the leaf's storage), as the reference's autograd
    does after a `p.data` update; the dense layers read the outputs they saved.  StyleGAN2's adjoint is dge_mapping_bwd or
    dge_mapping_bwd_wide by batch size (MAPPING_BWD_WIDE_MIN_BATCH, from the measurement in the README); StyleGAN1's
    MappingFunction keeps dge_mapping_bwd.
  * the tracker follows z; `independent` works as in W mode (the mapping is per-sample already); files are the W-mode set with the
    z row in models/id*-i*-z*.pt and models/z_all_*.pt [N, 512].

The file side of a group (dump_group, loss_txt_block, finish_group) and the group walk of main() (invert_folder, rows_plan) serve
embedding_v2_biggan too: its dumps differ in the two file-name patterns and in the Loss.txt block, its walk in labels and
img_all_*.pt.
"""
import argparse
import math
import os

import torch

from . import losses, ops, weight_cache
from .custom_adam import LREQAdam
from .embed_track import EVENT_LOSS, EVENT_NORM, EmbedTracker, tracker_rules, write_tracker_files  # noqa: F401 (re-exported)
from .embedding import select_launch
from .graph_step import GraphReplay
from .models import add_model_args, blur_encoder, load_lpips_weights

# per-generator defaults (embedding_v2_styleGAN1.py:195-209 + :118,128-131; embedding_v2_styleGAN2.py:214-232 + :136,153-166)
DEFAULTS = {
    1: dict(iterations=1501, lr=0.005, beta_1=0.0, beta=1e-3, norm_p=2, truncation=None),
    2: dict(iterations=2001, lr=0.005, beta_1=0.0, beta=3e-4, norm_p=2, truncation=0.7),
}
IMG_WEIGHTS = (1.0, 0.125 * 3, 0.125 * 5)
# mode "Z", StyleGAN2: smallest batch at which the mapping adjoint goes through dge_mapping_bwd_wide (None: never) - set from the
# measurement in the README section "Z-space inversion": the wide form is faster at every measured batch (1, 2, 4, 8)
MAPPING_BWD_WIDE_MIN_BATCH = 1


class _PNorm(torch.autograd.Function):
    """||w||_p (dge_latent_pnorm_fwd) with its gradient (dge_latent_pnorm_bwd)."""

    @staticmethod
    def forward(ctx, w, p):
        ctx.w, ctx.p = w.detach(), p
        ctx.n = ops.latent_pnorm(ctx.w, p)
        return ctx.n.clone()

    @staticmethod
    def backward(ctx, go):
        g = torch.zeros_like(ctx.w)
        ops.latent_pnorm_bwd(ctx.w, ctx.n, g, ctx.p, 1.0, gout=go.contiguous().float())
        return g, None


class _PNormRows(torch.autograd.Function):
    """||w[b]||_p for every row b -> [B] (dge_latent_pnorm_rows_fwd) with its gradient (dge_latent_pnorm_rows_bwd)."""

    @staticmethod
    def forward(ctx, w, p):
        ctx.w, ctx.p = w.detach(), p
        ctx.n = ops.latent_pnorm_rows(ctx.w, p)
        return ctx.n.clone()

    @staticmethod
    def backward(ctx, go):
        g = torch.zeros_like(ctx.w)
        ops.latent_pnorm_rows_bwd(ctx.w, ctx.n, g, ctx.p, 1.0, gout=go.contiguous().float())
        return g, None


class _WplusLerp(torch.autograd.Function):
    """avg + psi*(w - avg) on every row of a W+ code (dge_wplus_lerp / dge_wplus_lerp_bwd)."""

    @staticmethod
    def forward(ctx, w, avg, psi):
        ctx.psi = psi
        return ops.wplus_lerp(w.detach(), avg, psi)

    @staticmethod
    def backward(ctx, g):
        return ops.wplus_lerp_bwd(g, ctx.psi), None, None


class LatentEmbedStep(GraphReplay):
    fused_backward = True          # "pg": the generator backward with ops.pixelnorm_act_bwd (False: the composed launches, for timing)

    def __init__(self, G, E, lpips_model, mode="E", generator="sg2", lr=0.005, beta_1=0.0, beta=None, norm_p=2, truncation=None,
                 iterations=None, arm_iter=None, events_cap=256, seed=0, independent=False, Gm=None, mapping_bwd="auto"):
        if mode not in ("E", "W", "Z"):
            raise ValueError(f"mode must be 'E', 'W' or 'Z', got {mode!r}")
        if independent and mode == "E":
            raise ValueError("independent=True needs mode 'W' or 'Z': in mode 'E' one encoder is shared by the rows of a group")
        self.independent = bool(independent)
        if generator not in ("sg1", "sg2", "pg"):
            raise ValueError(f"generator must be 'sg1', 'sg2' or 'pg', got {generator!r}")
        if mode == "Z":
            if generator == "pg":
                raise ValueError("mode 'Z' is for StyleGAN1 / StyleGAN2: PGGAN's latent is z already (embedding_v2_pggan)")
            if generator == "sg1" and Gm is None:
                raise ValueError("mode 'Z' with generator 'sg1' needs the mapping network: pass Gm=stylegan1.Mapping")
            if mapping_bwd not in ("auto", "one", "wide"):
                raise ValueError(f"mapping_bwd must be 'auto', 'one' or 'wide', got {mapping_bwd!r}")
        self.Gm, self.mapping_bwd = Gm, mapping_bwd
        d = DEFAULTS[2 if generator == "sg2" else 1]          # "pg" (embedding_v2_pggan): StyleGAN1's defaults, rules and order
        self.G, self.E, self.lpips = G, E, lpips_model
        self.mode, self.generator = mode, generator
        self.lr, self.beta_1 = lr, beta_1
        self.beta = d["beta"] if beta is None else float(beta)
        self.norm_p = int(norm_p)
        self.psi = (d["truncation"] if truncation is None else float(truncation)) if generator == "sg2" else None
        self.iterations = d["iterations"] if iterations is None else int(iterations)
        self.rules = tracker_rules("sg2" if generator == "sg2" else "sg1", self.iterations)
        if arm_iter is not None:
            self.rules["arm_iter"] = int(arm_iter)
        self.events_cap, self.seed = int(events_cap), seed
        self.lod = G.layer_count - 1 if generator == "sg1" else None
        self.group = -1
        self.last = {}
        self.w1 = self._const2 = None
        self._tracker = EmbedTracker(self.rules, self.events_cap, rows=self.independent)
        if mode == "Z" and generator == "sg1":
            # the scripts' coefficients (embedding_v2_styleGAN1.py: 0.7 on the first half of the rows); without a centre Mapping
            # takes the plain broadcast whatever they are
            n = self._num_rows()
            self._coefs_m = torch.where(torch.arange(n).view(1, n, 1) < n // 2, 0.7, 1.0).float()
        if mode == "E":
            self.opt = LREQAdam([{"params": E.parameters()}], lr=lr, betas=(beta_1, 0.99), weight_decay=0)
            self._ckpt = {k: v.detach().clone() for k, v in E.state_dict().items()}
        else:
            for p in E.parameters():          # frozen: the encoder backward computes the data gradient only
                p.requires_grad_(False)
            E.eval()
            self.opt = None

    # ------------------------------------------------------------------ per image group
    def _num_rows(self):
        return self.E.layer_count * 2

    def _latent_shape(self, B):
        """Shape of the latent w1: the W+ code [B, rows, 512]; "pg": z [B, z_space_dim]."""
        if self.mode == "Z":
            return (B, 512)
        return (B, self.G.z_space_dim) if self.generator == "pg" else (B, self._num_rows(), 512)

    def _encode(self, imgs, noises):
        """(const, w) = E(imgs); "pg": E_PG has no const output -> (None, z)."""
        const, w = self.E(imgs, noises=noises)
        return (None if self.generator == "pg" else const), w

    def begin_image(self, imgs1, w_init=None, noises=None):
        """Start an image group: E mode re-loads the encoder checkpoint and clears the Adam state (embedding_v2_*.py: the
        per-group `E.load_state_dict`); W mode starts a fresh w1 (StyleGAN1: E(imgs1) detached, StyleGAN2: seeded randn or
        `w_init`) with a fresh Adam state.  The tracker's iteration counter and event log restart (in place: a captured
        iteration stays valid); the StyleGAN1 minima restart too, the StyleGAN2 ones carry over (independent mode: the minima of
        every row restart, and a StyleGAN2 row draws its start code from the seed of its image number).  `noises`: optional noise
        list of the StyleGAN1 W-mode E(imgs1) (parity runs)."""
        dev = imgs1.device
        B = imgs1.shape[0]
        self.group += 1
        shape = self._latent_shape(B)
        if self.mode == "E":
            self.E.load_state_dict(self._ckpt)
            weight_cache.written(self.E.parameters())
            self._reset_opt()
        else:
            with torch.no_grad():
                if self.mode == "Z" and self.generator == "sg1":          # const2 of the const term, a constant as in W mode
                    c0 = self.E(imgs1, noises=noises)[0]
                    if self._const2 is None or self._const2.shape != c0.shape:
                        self._const2 = torch.empty_like(c0)
                    self._const2.copy_(c0)
                if self.mode == "Z" and self.generator == "sg2":
                    wide = {"one": False, "wide": True}.get(self.mapping_bwd)
                    if wide is None:
                        wide = MAPPING_BWD_WIDE_MIN_BATCH is not None and B >= MAPPING_BWD_WIDE_MIN_BATCH
                    self.G.mapping.wide_bwd = wide
                if w_init is not None:
                    w0 = w_init.to(dev, torch.float32).reshape(shape)
                elif self.mode == "Z" and not self.independent:
                    w0 = torch.randn(shape, generator=torch.Generator().manual_seed(int(self.seed) + self.group))
                elif self.mode == "Z":
                    w0 = torch.cat([torch.randn((1,) + shape[1:], generator=torch.Generator().manual_seed(int(self.seed) + self.group * B + r))
                                    for r in range(B)])
                elif self.generator == "pg":
                    w0 = self._encode(imgs1, noises)[1]
                elif self.generator == "sg1":
                    c0, w0 = self.E(imgs1, noises=noises)
                    if self._const2 is None or self._const2.shape != c0.shape:
                        self._const2 = torch.empty_like(c0)
                    self._const2.copy_(c0)
                elif self.independent:
                    w0 = torch.cat([torch.randn((1,) + shape[1:], generator=torch.Generator().manual_seed(int(self.seed) + self.group * B + r))
                                    for r in range(B)])
                else:
                    gen = torch.Generator().manual_seed(int(self.seed) + self.group)
                    w0 = torch.randn(shape, generator=gen)
                if self.w1 is None or tuple(self.w1.shape) != shape or self.w1.device != dev:
                    if self.captured:
                        raise ValueError("LatentEmbedStep.begin_image: the captured iteration works on a different latent shape")
                    self.w1 = torch.zeros(shape, dtype=torch.float32, device=dev, requires_grad=True)
                    self.opt = LREQAdam([{"params": [self.w1]}], lr=self.lr, betas=(self.beta_1, 0.99), weight_decay=0)
                self.w1.copy_(w0)
            self._reset_opt()
        self._tracker.reset(shape, dev)

    # ------------------------------------------------------------------ one iteration
    def _generate(self, w1, noises):
        if self.generator == "sg1":
            return self.G.forward(w1, self.lod, noises=noises)
        if self.generator == "pg":          # (lod given: the generator does not read its `lod` buffer back, a captured iteration cannot)
            return self.G(w1, lod=0, fused_backward=self.fused_backward)["image"]
        syn = self.G.synthesis
        # (the synthesis backward reads its saved activations only, never wp: w1 itself may be the input when psi == 1)
        wt = w1 if self.psi == 1.0 else _WplusLerp.apply(w1, self.G.truncation.w_avg, self.psi)
        return syn(wt, randomize_noise=False)["image"]

    def _wp_of(self, z):
        """Mode "Z": wp = trunc(map(z)), differentiable w.r.t. z (StyleGAN2: dge_pixelnorm, eight dge_linear, dge_truncation)."""
        if self.generator == "sg1":
            return self.Gm(z, coefs_m=self._coefs_m)
        G = self.G
        return G.truncation(G.mapping(z)["w"], self.psi, G.num_layers)

    def _synthesise(self, wp, noises):
        """Mode "Z": imgs2 = G(wp), wp already truncated."""
        if self.generator == "sg1":
            return self.G.forward(wp, self.lod, noises=noises)
        return self.G.synthesis(wp, randomize_noise=False)["image"]

    def step(self, imgs1, noises=(None, None, None)):
        """One iteration; `noises` = optional (E(imgs1), G, E(imgs2)) noise lists for parity runs (StyleGAN2: G's is unused, the
        synthesis noise is its fixed buffers; W mode: E(imgs1)'s is unused).  Independent mode: the loss entries of the result
        (`loss_msiv`, `loss_w`, `loss_c1`, `norm`, `loss_mslv`, `w_norm`) are [B], `info_img` is [B,3,8]."""
        rows = self.independent
        if self.group < 0:
            raise RuntimeError("LatentEmbedStep.step: call begin_image() first")
        ops.zero_arena_begin(imgs1.device)
        if self.mode == "E":
            const2, w1 = self._encode(imgs1, noises[0])
        else:
            w1, const2 = self.w1, self._const2
        zmode = self.mode == "Z"
        wp = self._wp_of(w1) if zmode else None
        imgs2 = self._synthesise(wp, noises[1]) if zmode else self._generate(w1, noises[1])
        if self.generator != "sg2":
            const3, w2 = self._encode(imgs2, noises[2])
        image_loss, latent_loss = (losses.image_loss_tsa_rows, losses.space_loss_rows) if rows else (losses.image_loss_tsa, losses.space_loss)
        loss_msiv, info_img = image_loss(imgs1, imgs2, self.lpips, weights=IMG_WEIGHTS, grad_windows=(True, True, True))
        self.opt.zero_grad()
        loss_msiv.backward(retain_graph=True)
        self.opt.step()
        if self.generator == "sg2":
            const3, w2 = self._encode(imgs2, noises[2])
        wp_new = self._wp_of(w1) if zmode else None          # the direct term of phase 2 sees the updated code
        loss_w, info_w = latent_loss(wp_new if zmode else w1, w2, image_space=False)
        lat = loss_w
        loss_c1 = None
        if const2 is not None:
            loss_c1, info_c = latent_loss(const2, const3, image_space=False)
            lat = lat + loss_c1
        nrm = (_PNormRows if rows else _PNorm).apply(w1, self.norm_p)
        loss_mslv = lat * 0.01 + (nrm.sum() if rows else nrm) * self.beta
        self.opt.zero_grad()
        loss_mslv.backward()
        self.opt.step()
        w1d = w1.detach()
        if rows:      # the values of every row: the [B] columns of the info tensors (the scalars above are their sums over the rows)
            loss_msiv = info_img[:, 0, 0] * IMG_WEIGHTS[0] + info_img[:, 1, 0] * IMG_WEIGHTS[1] + info_img[:, 2, 0] * IMG_WEIGHTS[2]
            loss_w = info_w[:, 0].contiguous()
            loss_mslv = loss_w * 0.01 + nrm.detach() * self.beta
            if loss_c1 is not None:
                loss_c1 = info_c[:, 0].contiguous()
                loss_mslv = loss_mslv + loss_c1 * 0.01
        self._tracker.update(loss_msiv.detach(), w1d)
        ops.zero_arena_end()
        self.last = dict(w1=w1d, imgs2=imgs2.detach(), w2=w2.detach(), const2=const2.detach() if const2 is not None else None,
                         const3=const3.detach() if const3 is not None else None, loss_msiv=loss_msiv.detach(), info_img=info_img,
                         loss_w=loss_w.detach(), info_w=info_w, loss_c1=loss_c1.detach() if loss_c1 is not None else None, norm=nrm.detach(), loss_mslv=loss_mslv.detach(),
                         w_norm=self._tracker.l2)
        if zmode:
            self.last.update(wp=wp.detach(), wp_new=wp_new.detach())
        return self.last

    # ------------------------------------------------------------------ hipGraph replay of the iteration
    def capture(self, imgs1, noises=(None, None, None), warmup=GraphReplay.WARMUP):
        """`warmup` real iterations, then one recorded (not executed) iteration (GraphReplay._capture).  Adam's step factors come
        through graph_advance, the noise seed is a device scalar; in W mode the graph updates the static leaf w1 in place.
        begin_image() must have run for the group."""
        self._g_imgs1 = imgs1.detach().clone()
        self.opt.graph_begin(2, imgs1.device)          # two optimizer calls per iteration
        ops.noise_graph_begin(imgs1.device)
        self.graph_iteration = 0
        warm = {}

        def keep_last():    # results of the last executed iteration (the captured one is only recorded)
            if warmup:
                warm.update({k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.last.items()})
        out = self._capture(lambda: self.step(self._g_imgs1, noises), warmup, after_warmup=keep_last)
        self.last = warm
        return out

    def _graph_inputs(self, iteration):
        self.opt.graph_advance()
        ops.noise_graph_seed(iteration)

    def set_image(self, imgs1):
        """Copies a new image group into the static input of the captured iteration (call begin_image() for the group too)."""
        self._set_static("_g_imgs1", imgs1)

    def replay(self):
        self.last = super().replay()
        return self.last

    # ------------------------------------------------------------------ tracker read-out (one host read)
    def tracker(self):
        """The tracker's state on the host; independent mode: a list with one such read-out per row."""
        return self._tracker.read()


def group_plan(n_images, batch_size):
    """Independent mode: the groups of a folder of n_images as (first image number, rows kept) - every image is inverted, the last
    group may keep fewer rows than the batch holds."""
    return [(i, min(batch_size, n_images - i)) for i in range(0, n_images, batch_size)]


def padded_rows(first, batch_size, n_images):
    """Image numbers of the batch_size rows of the group that starts at image `first`: a short last group repeats its last image
    (the captured iteration keeps its shape); the caller discards those rows' outputs."""
    return [min(first + r, n_images - 1) for r in range(batch_size)]


def rows_plan(n_images, batch_size, labels=None):
    """The groups of the rows form: (first image number, rows kept, image number of every row, label of every row - None without
    `labels`) - a short last group repeats its last image and label."""
    plan = []
    for first, keep in group_plan(n_images, batch_size):
        idx = padded_rows(first, batch_size, n_images)
        plan.append((first, keep, idx, None if labels is None else [labels[i] for i in idx]))
    return plan


# ------------------------------------------------------------------ files of a group (shared with embedding_v2_biggan)
IMG_NAME, W_NAME = "id{n}_ep{i}-norm{norm:.2f}-imgLoss{loss:f}.jpg", "id{n}-i{k}-w{i}-norm{norm:f}-imgLoss{loss:f}.pt"
Z_NAME = "id{n}-i{k}-z{i}-norm{norm:f}-imgLoss{loss:f}.pt"          # mode "Z": the saved latent is the z row
LOSS_TXT_IMAGE = (("info_mask", "loss_small_info"), ("info_Gcam", "loss_medium_info"), ("info_imgs", "loss_imgs_info"))
LOSS_TXT_LATENT = (("info_w", "loss_w_info"), ("info_c2", "loss_c2_info"))


def loss_txt_block(f, num, i, infos, loss):
    """One Loss.txt block of embedding_v2_BigGAN.py:204-215 for image (group) `num` at iteration i; `infos`: the [8] info vectors
    (losses.space_loss) by result key - without the attention terms the small / medium lines are absent."""
    print("id_" + str(num) + "_____i_" + str(i), file=f)
    print("[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]", file=f)
    def lines(keys):
        for key, name in keys:
            if key in infos:
                print("%s: [[%s, %s, %s], %s, %s, %s, %s]" % ((name,) + tuple(float(x) for x in infos[key][1:8])), file=f)
    print("---------ImageSpace--------", file=f)
    lines(LOSS_TXT_IMAGE)
    print("---------LatentSpace--------", file=f)
    lines(LOSS_TXT_LATENT)
    print("Img_loss: %s" % loss, file=f)


def dump_group(st, imgs1, r, i, out_dir, group, keep=None, img_name=IMG_NAME, w_name=None, loss_txt=False):
    """The every-`save_every` dump of iteration i (norm and loss of all rows in one host read): the image pair and one w1 file per
    row; `loss_txt`: a Loss.txt block too.  Coupled form: one pair and one block for the group, named by `group`.  Independent
    form: a pair, a block and a w1 file for each of the first `keep` rows (default: all), named by the image number group * B + b,
    with that row's norm and loss.  `img_name` / `w_name`: format patterns of n (number), i, k (row of the file set), norm, loss
    (`w_name` None: W_NAME, Z_NAME for a step in mode "Z")."""
    from .infer import save_image_grid
    if w_name is None:
        w_name = Z_NAME if getattr(st, "mode", None) == "Z" else W_NAME
    B = imgs1.shape[0]
    vals = torch.stack((r["w_norm"], r["loss_msiv"])).reshape(2, -1).cpu()
    infos = {k: r[k].cpu() for k, _ in LOSS_TXT_IMAGE + LOSS_TXT_LATENT if k in r} if loss_txt else {}
    w1 = r["w1"].cpu()
    units = [(group, 0, slice(0, B))]          # (number, column of vals, rows of the batch)
    if st.independent:
        units = [(group * B + b, b, slice(b, b + 1)) for b in range(B if keep is None else keep)]
    for num, b, sl in units:
        names = dict(n=num, i=i, norm=float(vals[0, b]), loss=float(vals[1, b]))
        save_image_grid(torch.cat((imgs1[sl], r["imgs2"][sl])), os.path.join(out_dir, "imgs", img_name.format(**names)), nrow=2)
        if loss_txt:
            with open(os.path.join(out_dir, "Loss.txt"), "a+") as f:
                loss_txt_block(f, num, i, {k: (v[b] if st.independent else v) for k, v in infos.items()}, names["loss"])
        for k, row in enumerate(w1[sl]):
            torch.save(row.unsqueeze(0).clone(), os.path.join(out_dir, "models", w_name.format(k=k, **names)))


def finish_group(st, r, B, out_dir, group, keep=None):
    """The end of a group: the tracker read-out, its files with `out_dir` (independent form: per kept row, numbered group * B + b),
    and the result dict with the read-out under "tracker"."""
    tr = st.tracker()
    if out_dir is not None:
        models = os.path.join(out_dir, "models")
        if st.independent:
            for b in range(B if keep is None else keep):
                write_tracker_files(tr[b], group * B + b, models, out_dir)
        else:
            write_tracker_files(tr, group, models, out_dir)
    return dict(r, tracker=tr)


def invert_folder(invert, imgs, bs, independent, out, labels=None, save_imgs=False, all_name="w_all_%d.pt"):
    """The group walk of the CLIs: `invert(imgs1, group=g, **kw)` runs one group.  Coupled: the n // bs full groups, one line, one
    `summaries/<g>_rec.png` and w1[0] per group, models/w_all_<groups-1>.pt.  Independent: every image (rows_plan), a line and a w1
    per kept row, models/w_all_<n-1>.pt; `labels` (one class id per image) go to `invert` row by row.  `save_imgs`: the kept
    reconstructions too, as models/img_all_*.pt.  `all_name`: the pattern of the stacked latents' file (mode "Z": z_all_%d.pt)."""
    from .infer import save_image_grid
    n = imgs.shape[0]
    plan = rows_plan(n, bs, labels) if independent else [(g * bs, bs, list(range(g * bs, (g + 1) * bs)), None) for g in range(n // bs)]
    w_all, img_all = [], []
    for g, (first, keep, idx, lab) in enumerate(plan):
        kw = dict(keep=keep, **({} if lab is None else {"labels": lab})) if independent else {}
        r = invert(imgs[idx].contiguous(), group=g, **kw)
        vals = torch.stack((r["loss_msiv"], r["w_norm"])).reshape(2, -1).cpu()
        trs = r["tracker"] if independent else [r["tracker"]]
        for b in range(keep if independent else 1):
            who = ("image %d" % (first + b) + ("" if lab is None else " (label %d)" % lab[b])) if independent else "group %d" % g
            print("%s: loss_msiv %.5f  w_norm %.4f  events %d" % (who, float(vals[0, b]), float(vals[1, b]), len(trs[b]["events"])))
            w_all.append(r["w1"][b].clone().cpu())
            if save_imgs:
                img_all.append(r["imgs2"][b].clone().cpu())
        save_image_grid(r["imgs2"][:keep], os.path.join(out, "summaries", "%s_rec.png" % str(g).rjust(5, "0")), nrow=bs)
    if w_all:
        torch.save(torch.stack(w_all, dim=0), os.path.join(out, "models", all_name % (len(w_all) - 1)))
        if save_imgs:
            torch.save(torch.stack(img_all, dim=0), os.path.join(out, "models", "img_all_%d.pt" % (len(w_all) - 1)))


def invert_v2(st, imgs1, iterations, launch="graph", save_every=100, out_dir=None, group=0, w_init=None, keep=None):
    """`iterations` iterations on one image group.  launch="graph" captures the iteration once (its warm-up iteration is a real one)
    and replays it; later groups go through set_image.  With `out_dir` the reference's every-`save_every` dumps (dump_group: image
    pair, per-row w1) are written and, at the end, the trackers' files (finish_group).  Returns the last result dict with the tracker
    read-out under "tracker".  Independent mode: files carry the image number group*B + b and that row's norm and loss; only the
    first `keep` rows (default: all) are written, and "tracker" is the list of per-row read-outs."""
    st.begin_image(imgs1, w_init=w_init)
    if launch not in ("graph", "eager"):
        raise ValueError(f"launch must be 'graph' or 'eager', got {launch!r}")
    run, done = select_launch(st, imgs1, launch)
    r = st.last
    dumps = out_dir is not None and save_every
    if done and dumps:
        dump_group(st, imgs1, r, 0, out_dir, group, keep)          # iteration 0 ran as capture()'s warm-up
    for i in range(done, iterations):
        r = run()
        if dumps and i % save_every == 0:
            dump_group(st, imgs1, r, i, out_dir, group, keep)
    return finish_group(st, r, imgs1.shape[0], out_dir, group, keep)


ENCODERS = ("blur", "be")


def _be_encoder(img_size, start_features, compute_dtype, device, maxf):
    """E.BE (encoder.BE, the encoder E_align trains) sized for `img_size`: its checkpoints load unchanged."""
    from .encoder import BE
    return BE(start_features, maxf or 512, int(math.log2(img_size) - 1), compute_dtype=compute_dtype).to(device)


def build_models_v2(mtype, img_size=1024, start_features=16, compute_dtype="bf16", device="cuda", seed=0, lpips=True,
                    fmaps_base=None, fmaps_max=None, enc_maxf=None, encoder="blur"):
    """mtype 1: StyleGAN1 Gs + E_Blur (embedding.build_models); mtype 2: StyleGAN2Generator (eval, frozen, fixed noise) +
    BlurBE(layer_count = log2(res) - 1) - 18 W+ rows at 1024^2, 10 at 64^2.  Seeded random-init weights.
    encoder="be": E.BE(start_features, enc_maxf or 512, log2(res) - 1) in place of E_Blur, for both mtypes."""
    from .lpips import LPIPS
    if encoder not in ENCODERS:
        raise ValueError(f"embedding_v2: encoder must be one of {ENCODERS}, got {encoder!r}")
    torch.manual_seed(seed)
    if mtype == 1:
        from .embedding import build_models
        G, E, LP = build_models(img_size, start_features, compute_dtype, device=device, seed=seed)
        if encoder == "be":
            E = _be_encoder(img_size, start_features, compute_dtype, device, enc_maxf)
        return G, E, (LP if lpips else None)
    if mtype != 2:
        raise ValueError("embedding_v2: --mtype 1 (StyleGAN1) or 2 (StyleGAN2); BigGAN / PGGAN inversion is not offered")
    from .stylegan2_generator import StyleGAN2Generator
    kw = {k: v for k, v in (("fmaps_base", fmaps_base), ("fmaps_max", fmaps_max)) if v is not None}
    G = StyleGAN2Generator(img_size, compute_dtype=compute_dtype, **kw).to(device)
    G.eval()
    for p in G.parameters():
        p.requires_grad_(False)
    if encoder == "be":
        E = _be_encoder(img_size, start_features, compute_dtype, device, enc_maxf)
    else:
        E = blur_encoder(img_size, start_features, compute_dtype, device, maxf=enc_maxf or 512)
    LP = LPIPS(compute_dtype=compute_dtype).to(device) if lpips else None
    return G, E, LP


def build_mapping_sg1(G, device="cuda", seed=0):
    """Mode "Z", mtype 1: the StyleGAN1 mapping network for the synthesis `G` (frozen, seeded random-init, no truncation centre)."""
    from .stylegan1 import Mapping
    torch.manual_seed(seed + 1)
    Gm = Mapping(num_layers=2 * G.layer_count, mapping_layers=8, latent_size=512, dlatent_size=512, mapping_fmaps=512).to(device)
    for p in Gm.parameters():
        p.requires_grad_(False)
    return Gm


def load_checkpoints(G, E, mtype, gan=None, enc=None, Gm=None):
    """The checkpoint containers of models.load_models: mtype 2 a dict holding `generator_smooth` (or `generator`), mtype 1 a
    directory with Gs_dict.pth (and, for `Gm`, Gm_dict.pth and - optional - center_tensor.pt); the encoder a bare state_dict."""
    if gan and Gm is not None:
        Gm.load_state_dict(torch.load(gan + "Gm_dict.pth", map_location="cpu"))
        if os.path.exists(gan + "center_tensor.pt"):
            Gm.buffer1 = torch.load(gan + "center_tensor.pt", map_location="cpu")
    if gan:
        if mtype == 2:
            ckpt = torch.load(gan, map_location="cpu")
            G.load_state_dict(ckpt["generator_smooth"] if "generator_smooth" in ckpt else ckpt["generator"])
        else:
            G.load_state_dict(torch.load(gan + "Gs_dict.pth", map_location="cpu"))
    if enc:
        E.load_state_dict(torch.load(enc, map_location="cpu"))


# ------------------------------------------------------------------ CLI
def strict_bool(s):
    v = str(s).strip().lower()
    if v in ("true", "1", "yes"):
        return True
    if v in ("false", "0", "no"):
        return False
    raise argparse.ArgumentTypeError(f"expected true or false, got {s!r}")


def make_parser():
    p = argparse.ArgumentParser(description="real-image inversion (embedding_v2_styleGAN1.py / embedding_v2_styleGAN2.py)")
    p.add_argument("--iterations", type=int, default=None, help="default: 1501 (mtype 1), 2001 (mtype 2)")
    p.add_argument("--lr", type=float, default=None, help="default 0.005")
    p.add_argument("--beta_1", type=float, default=None, help="default 0.0")
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--experiment_dir", default=None)
    add_model_args(p)
    p.set_defaults(mtype=1)
    p.add_argument("--img_dir", default="./real_imgs/", help="a directory of images or a .pt tensor in [0,1]")
    p.add_argument("--optimizeE", type=strict_bool, default=True, help="true: fine-tune the encoder; false: optimise W+ directly")
    p.add_argument("--space", choices=("w", "z"), default="w",
                   help="with --optimizeE false: optimise the W+ code (w) or z in front of the mapping network (z; --mtype 1 or 2)")
    p.add_argument("--independent", type=strict_bool, default=False,
                   help="true (with --optimizeE false): every image of a batch is an inversion of its own, equal to its batch-1 run")
    p.add_argument("--encoder", choices=ENCODERS, default="blur",
                   help="blur: E_Blur; be: E.BE, the encoder E_align trains (--checkpoint_dir_E then takes its checkpoints)")
    p.add_argument("--beta", type=float, default=None, help="weight of ||w1||_p: default 1e-3 (mtype 1), 3e-4 (mtype 2)")
    p.add_argument("--norm_p", type=int, default=None, help="p of ||w1||_p (default 2)")
    p.add_argument("--truncation", type=float, default=None, help="StyleGAN2: psi of avg + psi*(w1 - avg) (default 0.7; 1: none)")
    p.add_argument("--launch", choices=("eager", "graph"), default="graph")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--save_every", type=int, default=100)
    p.add_argument("--vgg_weights", default=None)
    p.add_argument("--lpips_weights", default=None)
    p.add_argument("--allow_standin_lpips", action="store_true")
    p.add_argument("--deterministic", action="store_true")
    return p


def parse_args(argv=None):
    """Parsed flags with the per-`--mtype` defaults filled in."""
    args = make_parser().parse_args(argv)
    if args.space == "z":
        if args.optimizeE:
            raise SystemExit("embedding_v2: --space z needs --optimizeE false (z is optimised against the frozen encoder)")
        if args.mtype not in (1, 2):
            raise SystemExit("embedding_v2: --space z is for --mtype 1 (StyleGAN1) or 2 (StyleGAN2); PGGAN and BigGAN optimise z already")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("embedding_v2: --space z runs in one process (WORLD_SIZE > 1 is not supported)")
    if args.mtype not in DEFAULTS:
        raise SystemExit("embedding_v2: --mtype must be 1 (StyleGAN1) or 2 (StyleGAN2)")
    if args.independent and args.optimizeE:
        raise SystemExit("embedding_v2: --independent true needs --optimizeE false (the fine-tuned encoder is shared by a group)")
    for k, v in DEFAULTS[args.mtype].items():
        if getattr(args, k, None) is None:
            setattr(args, k, v)
    return args


def _load_imgs(path, size, device):
    if path.endswith(".pt"):
        return (torch.load(path, map_location="cpu").float() * 2 - 1).to(device)
    from .infer import load_images
    names = sorted(n for n in os.listdir(path) if n.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")))
    return load_images([os.path.join(path, n) for n in names], size, bicubic=True, device=device)


def main(argv=None):
    args = parse_args(argv)
    if args.deterministic:
        ops.set_deterministic(True)
    dev = "cuda"
    G, E, LP = build_models_v2(args.mtype, args.img_size, args.start_features, args.compute_dtype, device=dev, seed=args.seed,
                               fmaps_base=args.fmaps_base, fmaps_max=args.fmaps_max, enc_maxf=args.enc_maxf, encoder=args.encoder)
    zspace = args.space == "z"
    Gm = build_mapping_sg1(G, dev, args.seed) if zspace and args.mtype == 1 else None
    load_checkpoints(G, E, args.mtype, args.checkpoint_dir_GAN, args.checkpoint_dir_E, Gm=Gm)
    load_lpips_weights(LP, args.vgg_weights, args.lpips_weights, allow_standin=args.allow_standin_lpips)
    out = args.experiment_dir or "./realimg_embedding_result/7"
    for sub in ("", "imgs", "models", "summaries"):
        os.makedirs(os.path.join(out, sub), exist_ok=True)
    imgs = _load_imgs(args.img_dir, args.img_size, dev)
    st = LatentEmbedStep(G, E, LP, mode="E" if args.optimizeE else ("Z" if zspace else "W"), Gm=Gm, generator="sg1" if args.mtype == 1 else "sg2", lr=args.lr,
                         beta_1=args.beta_1, beta=args.beta, norm_p=args.norm_p, truncation=args.truncation,
                         iterations=args.iterations, seed=args.seed, independent=args.independent)
    invert_folder(lambda imgs1, **kw: invert_v2(st, imgs1, args.iterations, launch=args.launch, save_every=args.save_every, out_dir=out, **kw),
                  imgs, args.batch_size, args.independent, out, all_name="z_all_%d.pt" if zspace else "w_all_%d.pt")
    return st


if __name__ == "__main__":
    main()
