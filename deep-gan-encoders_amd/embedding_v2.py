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

What differs between the generator kinds "sg1", "sg2" and "pg" is one table (KINDS): the defaults and tracker rules, the latent
shape, how E and G are called, whether E(imgs2) runs before or after the phase-1 step, and where the W-mode start code comes
from.  Kind "pg" (embedding_v2_pggan.PGEmbedStep: PGGAN + E_PG) runs the iteration on z [B, z_space_dim] in StyleGAN1's order
and with its defaults and rules; E_PG has no const output: const2 / const3 / loss_c1 are None.  The constructor tail, the start of
a group, the optimiser phase and the hipGraph plumbing are embed_step.TwoPhaseEmbedStep's, shared with embedding_v2_biggan.

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

Noise optimisation (`optimize_noise`, --optimize_noise true; StyleGAN2, mode "W", one process): the per-layer noise maps of the
synthesis network become free variables beside the W+ code, as in StyleGAN2's own projector.
  * the maps start at the generator's `layer{i}.noise` buffers - one shared set [1,res,res] per layer, or a copy per row
    [B,res,res] with `independent` - and live in one flat f32 buffer (noise_maps.NoiseMaps, the step's `noise`; shared with the
    projector) with one LREQAdam of its own (`nopt`: lr `noise_lr` or lr, its own step count); begin_image resets the maps and
    that Adam state in place.
  * phase 1 back-propagates loss_msiv + noise_reg * sum reg(map) (the projector's regulariser, dge_noise_reg): the synthesis
    backward writes each map's image-loss gradient (dge_s2_noise_grad) into the flat gradient buffer and the regulariser's
    gradient is added to it.  loss_msiv, the tracker and every logged loss stay the image loss alone; reg is logged as `noise_reg`
    ([B] in rows form).
  * the maps take one Adam step per iteration from that phase-1 gradient and are renormalised to zero mean and unit mean square
    (dge_noise_normalize).  Phase 2 launches no noise pass (SynthesisModule.noise_grad_enabled is off for its backward) and moves
    no map.  The step and the renormalisation are ISSUED behind the phase-2 backward: the retained synthesis graph reads its
    noise operand by reference (the demodulation sums reconstruct yraw*d + bias as z - ns*noise), so a map may not move under
    it.  Nothing in phase 2 depends on the updated maps, so the results are those of stepping between the phases.
  * finish_group also writes models/id{n}-noise.pt, the list of maps of that image (each [1,res,res]); they reload into
    StyleGAN2Generator.synthesis(wp, noises=...).

The loop over the iterations of a group (invert_group), its file side (dump_group, loss_txt_block, finish_group), the group walk
of main() (invert_folder, rows_plan) and the common part of the command lines (add_inversion_args, open_run, run_inversion) serve
embedding_v2_pggan and embedding_v2_biggan too: their dumps differ in the file-name patterns and in the Loss.txt block, BigGAN's
walk in labels and img_all_*.pt.
"""
import argparse
import collections
import math
import os

import torch

from . import losses, ops
from .custom_adam import LREQAdam
from .embed_step import TwoPhaseEmbedStep, several_processes
from .embed_track import EVENT_LOSS, EVENT_NORM, tracker_rules, write_tracker_files  # noqa: F401 (re-exported)
from .embedding import iterate
from .models import add_model_args, blur_encoder, load_lpips_weights
from .noise_maps import NoiseMaps, save_noise_rows

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
    """||w||_p (dge_latent_pnorm_fwd) with its gradient (dge_latent_pnorm_bwd); `rows`: ||w[b]||_p for every row b -> [B]
    (dge_latent_pnorm_rows_fwd / dge_latent_pnorm_rows_bwd)."""

    @staticmethod
    def forward(ctx, w, p, rows):
        ctx.w, ctx.p, ctx.rows = w.detach(), p, rows
        ctx.n = (ops.latent_pnorm_rows if rows else ops.latent_pnorm)(ctx.w, p)
        return ctx.n.clone()

    @staticmethod
    def backward(ctx, go):
        g = torch.zeros_like(ctx.w)
        (ops.latent_pnorm_rows_bwd if ctx.rows else ops.latent_pnorm_bwd)(ctx.w, ctx.n, g, ctx.p, 1.0, gout=go.contiguous().float())
        return g, None, None


class _WplusLerp(torch.autograd.Function):
    """avg + psi*(w - avg) on every row of a W+ code (dge_wplus_lerp / dge_wplus_lerp_bwd)."""

    @staticmethod
    def forward(ctx, w, avg, psi):
        ctx.psi = psi
        return ops.wplus_lerp(w.detach(), avg, psi)

    @staticmethod
    def backward(ctx, g):
        return ops.wplus_lerp_bwd(g, ctx.psi), None, None


# What a generator kind is to LatentEmbedStep.  `defaults`: row of DEFAULTS; `rules`: name for tracker_rules; `latent_shape(st, B)`;
# `encode(st, imgs, noises)` -> (const, w); `generate(st, code, noises, truncate)` -> imgs2; `encode_first`: E(imgs2) runs before
# the phase-1 step (StyleGAN1's order) or after it; `start`: the W-mode start code is E(imgs1) ("encoder") or a seeded randn;
# `own_mapping`: mode "Z" maps z with the step's Gm (StyleGAN1) instead of G.mapping and G.truncation.
Kind = collections.namedtuple("Kind", "defaults rules latent_shape encode generate encode_first start own_mapping", defaults=(False,))


def _wplus_shape(st, B):
    return (B, st._num_rows(), 512)


def _encode(st, imgs, noises):
    return st.E(imgs, noises=noises)


def _generate_sg1(st, w, noises, truncate):
    return st.G.forward(w, st.G.layer_count - 1, noises=noises)


def _generate_sg2(st, w, noises, truncate):
    # (the synthesis backward reads its saved activations only, never wp: w itself may be the input when psi == 1)
    wt = w if st.psi == 1.0 or not truncate else _WplusLerp.apply(w, st.G.truncation.w_avg, st.psi)
    if st.optimize_noise:
        return st.G.synthesis(wt, randomize_noise=False, noises=st.noise.maps, noise_grad_out=st.noise.grads)["image"]
    return st.G.synthesis(wt, randomize_noise=False)["image"]


def _generate_pg(st, z, noises, truncate):          # (lod given: the generator does not read its `lod` buffer back, a captured iteration cannot)
    return st.G(z, lod=0, fused_backward=st.fused_backward)["image"]


KINDS = {
    "sg1": Kind(1, "sg1", _wplus_shape, _encode, _generate_sg1, encode_first=True, start="encoder", own_mapping=True),
    "sg2": Kind(2, "sg2", _wplus_shape, _encode, _generate_sg2, encode_first=False, start="randn"),
    # PGGAN + E_PG (embedding_v2_pggan): StyleGAN1's defaults, rules and order; E_PG has no const output -> (None, z)
    "pg": Kind(1, "sg1", lambda st, B: (B, st.G.z_space_dim), lambda st, imgs, noises: (None, _encode(st, imgs, noises)[1]), _generate_pg,
               encode_first=True, start="encoder"),
}


def seeded_start(shape, seed, group, rows):
    """The seeded start code of group `group`: randn(shape) from manual_seed(seed + group); `rows`: row r is the randn(1, ...) from
    manual_seed(seed + group * B + r), the draw a batch-1 run makes for image number group * B + r."""
    def draw(number, shp):
        return torch.randn(shp, generator=torch.Generator().manual_seed(int(seed) + number))
    if not rows:
        return draw(group, shape)
    return torch.cat([draw(group * shape[0] + r, (1,) + shape[1:]) for r in range(shape[0])])


class LatentEmbedStep(TwoPhaseEmbedStep):
    MODES = ("E", "W", "Z")
    fused_backward = True          # "pg": the generator backward with ops.pixelnorm_act_bwd (False: the composed launches, for timing)

    def __init__(self, G, E, lpips_model, mode="E", generator="sg2", lr=0.005, beta_1=0.0, beta=None, norm_p=2, truncation=None,
                 iterations=None, arm_iter=None, events_cap=256, seed=0, independent=False, Gm=None, mapping_bwd="auto",
                 optimize_noise=False, noise_reg=1e5, noise_lr=None):
        if optimize_noise:
            why = noise_refusal(generator == "sg2", mode == "E", mode == "Z", several_processes())
            if why:
                raise ValueError("LatentEmbedStep: " + why)
        if independent and mode == "E":
            raise ValueError("independent=True needs mode 'W' or 'Z': in mode 'E' one encoder is shared by the rows of a group")
        if generator not in KINDS:
            raise ValueError(f"generator must be 'sg1', 'sg2' or 'pg', got {generator!r}")
        if mode == "Z":
            if generator == "pg":
                raise ValueError("mode 'Z' is for StyleGAN1 / StyleGAN2: PGGAN's latent is z already (embedding_v2_pggan)")
            if generator == "sg1" and Gm is None:
                raise ValueError("mode 'Z' with generator 'sg1' needs the mapping network: pass Gm=stylegan1.Mapping")
            if mapping_bwd not in ("auto", "one", "wide"):
                raise ValueError(f"mapping_bwd must be 'auto', 'one' or 'wide', got {mapping_bwd!r}")
        self.generator, self.kind = generator, KINDS[generator]
        d = DEFAULTS[self.kind.defaults]
        super().__init__(G, E, lpips_model, mode, self.kind.rules, lr, beta_1, d["iterations"] if iterations is None else iterations,
                         arm_iter, events_cap, independent)
        self.Gm, self.mapping_bwd, self.seed = Gm, mapping_bwd, seed
        self.beta = d["beta"] if beta is None else float(beta)
        self.norm_p = int(norm_p)
        self.psi = None if d["truncation"] is None else (d["truncation"] if truncation is None else float(truncation))
        self._const2 = None
        self.optimize_noise, self.noise_reg, self.noise_lr = bool(optimize_noise), float(noise_reg), noise_lr
        self.noise = self.nopt = None          # the NoiseMaps owner and its LREQAdam: from the first group with optimize_noise
        if mode == "Z" and self.kind.own_mapping:
            # the scripts' coefficients (embedding_v2_styleGAN1.py: 0.7 on the first half of the rows); without a centre Mapping
            # takes the plain broadcast whatever they are
            n = self._num_rows()
            self._coefs_m = torch.where(torch.arange(n).view(1, n, 1) < n // 2, 0.7, 1.0).float()
        if mode != "E":
            E.eval()

    # ------------------------------------------------------------------ per image group
    def _num_rows(self):
        return self.E.layer_count * 2

    def _latent_shape(self, B):
        """Shape of the latent w1: the W+ code [B, rows, 512]; "pg": z [B, z_space_dim]; mode "Z": z [B, 512]."""
        return (B, 512) if self.mode == "Z" else self.kind.latent_shape(self, B)

    def _start_code(self, imgs1, shape, noises, needed):
        """begin_image (TwoPhaseEmbedStep) for a frozen encoder: w1 starts from E(imgs1) detached (StyleGAN1, PGGAN) or a seeded
        randn (StyleGAN2, mode "Z"), unless `w_init` is given (`needed` False).  The StyleGAN1 minima of the tracker restart with
        the group, the StyleGAN2 ones carry over (independent mode: the minima of every row restart, and a row draws its start code
        from the seed of its image number).  `noises`: optional noise list of the E(imgs1) below (parity runs)."""
        zmode = self.mode == "Z"
        encoded = needed and not zmode and self.kind.start == "encoder"
        w0 = None
        if encoded or (zmode and self.kind.own_mapping):          # (mode "Z", StyleGAN1: for const2 alone, a constant as in W mode)
            c0, w0 = self.kind.encode(self, imgs1, noises)
            if c0 is not None:
                if self._const2 is None or self._const2.shape != c0.shape:
                    self._const2 = torch.empty_like(c0)
                self._const2.copy_(c0)
        if zmode and not self.kind.own_mapping:
            wide = {"one": False, "wide": True}.get(self.mapping_bwd)
            if wide is None:
                wide = MAPPING_BWD_WIDE_MIN_BATCH is not None and shape[0] >= MAPPING_BWD_WIDE_MIN_BATCH
            self.G.mapping.wide_bwd = wide
        return w0 if encoded or not needed else seeded_start(shape, self.seed, self.group, self.independent)

    # ------------------------------------------------------------------ the noise maps (optimize_noise)
    def begin_image(self, imgs1, w_init=None, noises=None, **group_kw):
        """With optimize_noise, the maps of the new group too: the generator's buffers, copied per row in independent mode, into the
        NoiseMaps owner (allocated once per shape and device, with the LREQAdam over its flat leaf); that Adam state is cleared in place."""
        super().begin_image(imgs1, w_init=w_init, noises=noises, **group_kw)
        if not self.optimize_noise:
            return
        Bn = imgs1.shape[0] if self.independent else 1
        if self.noise is None or not self.noise.fits(Bn, self.w1.device):
            if self.captured:
                raise ValueError("LatentEmbedStep.begin_image: the captured iteration works on other noise maps")
            self.noise = NoiseMaps(self.G.synthesis, Bn, imgs1.device)
            self.nopt = LREQAdam([{"params": [self.noise.flat]}], lr=self.lr if self.noise_lr is None else self.noise_lr,
                                 betas=(self.beta_1, 0.99), weight_decay=0)
        self.noise.reset()
        self.nopt.graph_reset()

    def _noise_step(self):
        """One LREQAdam step of the maps from the phase-1 gradient, then the renormalisation."""
        self.noise.hand_grad()
        self.nopt.step()
        self.noise.flat.grad = None
        self.noise.normalize()

    def _graph_opts(self):
        """Two calls of `opt` per iteration; the maps' optimiser makes one, with its own step count."""
        return [(self.opt, 2)] + ([(self.nopt, 1)] if self.optimize_noise else [])

    # ------------------------------------------------------------------ one iteration
    def _generate(self, w1, noises):
        return self.kind.generate(self, w1, noises, truncate=True)

    def _wp_of(self, z):
        """Mode "Z": wp = trunc(map(z)), differentiable w.r.t. z (StyleGAN2: dge_pixelnorm, eight dge_linear, dge_truncation)."""
        if self.kind.own_mapping:
            return self.Gm(z, coefs_m=self._coefs_m)
        G = self.G
        return G.truncation(G.mapping(z)["w"], self.psi, G.num_layers)

    def _synthesise(self, wp, noises):
        """Mode "Z": imgs2 = G(wp), wp already truncated."""
        return self.kind.generate(self, wp, noises, truncate=False)

    def step(self, imgs1, noises=(None, None, None)):
        """One iteration; `noises` = optional (E(imgs1), G, E(imgs2)) noise lists for parity runs (StyleGAN2: G's is unused, the
        synthesis noise is its fixed buffers; W mode: E(imgs1)'s is unused).  Independent mode: the loss entries of the result
        (`loss_msiv`, `loss_w`, `loss_c1`, `norm`, `loss_mslv`, `w_norm`) are [B], `info_img` is [B,3,8]."""
        rows, kind = self.independent, self.kind
        if self.group < 0:
            raise RuntimeError("LatentEmbedStep.step: call begin_image() first")
        ops.zero_arena_begin(imgs1.device)
        if self.mode == "E":
            const2, w1 = kind.encode(self, imgs1, noises[0])
        else:
            w1, const2 = self.w1, self._const2
        zmode = self.mode == "Z"
        wp = self._wp_of(w1) if zmode else None
        imgs2 = self._synthesise(wp, noises[1]) if zmode else self._generate(w1, noises[1])
        if kind.encode_first:
            const3, w2 = kind.encode(self, imgs2, noises[2])
        image_loss, latent_loss = (losses.image_loss_tsa_rows, losses.space_loss_rows) if rows else (losses.image_loss_tsa, losses.space_loss)
        loss_msiv, info_img = image_loss(imgs1, imgs2, self.lpips, weights=IMG_WEIGHTS, grad_windows=(True, True, True))
        self._opt_phase(loss_msiv, retain_graph=True)
        if self.optimize_noise:          # phase 1's loss is loss_msiv + noise_reg * sum reg: the regulariser's gradient joins the image loss's
            self.noise.add_reg(self.noise_reg)
        if not kind.encode_first:
            const3, w2 = kind.encode(self, imgs2, noises[2])
        wp_new = self._wp_of(w1) if zmode else None          # the direct term of phase 2 sees the updated code
        loss_w, info_w = latent_loss(wp_new if zmode else w1, w2, image_space=False)
        lat = loss_w
        loss_c1 = None
        if const2 is not None:
            loss_c1, info_c = latent_loss(const2, const3, image_space=False)
            lat = lat + loss_c1
        nrm = _PNorm.apply(w1, self.norm_p, rows)
        loss_mslv = lat * 0.01 + (nrm.sum() if rows else nrm) * self.beta
        if self.optimize_noise:
            self.G.synthesis.noise_grad_enabled = False          # phase 2 through the retained graph: d/dw1 alone
            try:
                self._opt_phase(loss_mslv)
            finally:
                self.G.synthesis.noise_grad_enabled = True
            self._noise_step()
        else:
            self._opt_phase(loss_mslv)
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
        if self.optimize_noise:          # the maps behind this iteration's step, its phase-1 gradients (valid until the next backward), reg
            self.last.update(noises=self.noise.detached(), noise_grads=self.noise.grads, noise_reg=self.noise.reg)
        return self.last


def noise_refusal(sg2, mode_e, mode_z, several):
    """Why noise optimisation is not offered for a configuration (None: it is): the step's and the command line's one rule."""
    if not sg2:
        return "noise optimisation is for StyleGAN2 (--mtype 2): the other generators' noise inputs have no gradient pass"
    if mode_e:
        return "noise optimisation needs --optimizeE false: the maps are optimised beside the W+ code, not beside the encoder"
    if mode_z:
        return "noise optimisation is not offered with --space z: it runs beside the W+ code (mode W)"
    if several:
        return "noise optimisation runs in one process (WORLD_SIZE > 1 is not supported)"
    return None


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
        if getattr(st, "optimize_noise", False):          # the maps of every image, as synthesis(noises=...) takes them
            rows = range(B if keep is None else keep) if st.independent else [0]          # (coupled form: the one shared set)
            save_noise_rows([m.cpu() for m in r["noises"]], rows, [group * B + b for b in rows] if st.independent else [group], models)
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


def invert_group(st, imgs1, iterations, launch, save_every, out_dir, group, keep, begin_kw={}, dump_kw={}, infos=None):
    """The loop of invert_v2, embedding_v2_pggan.invert_pg and embedding_v2_biggan.invert_big: begin_image(imgs1, **begin_kw),
    `iterations` iterations through `launch`, a dump_group(..., **dump_kw) at every `save_every`-th with `out_dir`, finish_group.
    `infos(r)`: the result dict with the info vectors under the keys loss_txt_block prints."""
    st.begin_image(imgs1, **begin_kw)
    r = st.last
    for i, r in iterate(st, imgs1, iterations, launch):
        if out_dir is not None and save_every and i % save_every == 0:
            dump_group(st, imgs1, r if infos is None else infos(r), i, out_dir, group, keep, **dump_kw)
    return finish_group(st, r, imgs1.shape[0], out_dir, group, keep)


def invert_v2(st, imgs1, iterations, launch="graph", save_every=100, out_dir=None, group=0, w_init=None, keep=None):
    """`iterations` iterations on one image group.  launch="graph" captures the iteration once (its warm-up iteration is a real one)
    and replays it; later groups go through set_image.  With `out_dir` the reference's every-`save_every` dumps (dump_group: image
    pair, per-row w1) are written and, at the end, the trackers' files (finish_group).  Returns the last result dict with the tracker
    read-out under "tracker".  Independent mode: files carry the image number group*B + b and that row's norm and loss; only the
    first `keep` rows (default: all) are written, and "tracker" is the list of per-row read-outs."""
    return invert_group(st, imgs1, iterations, launch, save_every, out_dir, group, keep, dict(w_init=w_init))


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
            load_generator_smooth(G, gan)
        else:
            G.load_state_dict(torch.load(gan + "Gs_dict.pth", map_location="cpu"))
    if enc:
        E.load_state_dict(torch.load(enc, map_location="cpu"))


def load_generator_smooth(G, path):
    """The generator container of models.load_models for --mtype 2 and 3: a dict holding `generator_smooth` (or `generator`)."""
    ckpt = torch.load(path, map_location="cpu")
    G.load_state_dict(ckpt["generator_smooth"] if "generator_smooth" in ckpt else ckpt["generator"])


# ------------------------------------------------------------------ CLI (the common part serves embedding_v2_pggan / _biggan too)
def strict_bool(s):
    v = str(s).strip().lower()
    if v in ("true", "1", "yes"):
        return True
    if v in ("false", "0", "no"):
        return False
    raise argparse.ArgumentTypeError(f"expected true or false, got {s!r}")


def _refuse(msg):
    """argparse type of a flag that is not offered: any value is an error with `msg`."""
    def parse(_):
        raise argparse.ArgumentTypeError(msg)
    return parse


def add_inversion_args(p, defaults, mtype, img_dir, latent, launch=True, helps={}):
    """The flags every inversion CLI has.  `defaults`: of --iterations / --lr / --beta_1 / --batch_size (absent: None, filled in later;
    batch_size 1), `helps`: their help texts; `latent`: what --optimizeE false optimises, for its help text; `launch`: offer --launch."""
    for name, typ in (("iterations", int), ("lr", float), ("beta_1", float)):
        p.add_argument("--" + name, type=typ, default=defaults.get(name), help=helps.get(name))
    p.add_argument("--batch_size", type=int, default=defaults.get("batch_size", 1))
    p.add_argument("--experiment_dir", default=None)
    add_model_args(p)
    p.set_defaults(mtype=mtype)
    p.add_argument("--img_dir", default=img_dir, help="a directory of images or a .pt tensor in [0,1]")
    p.add_argument("--optimizeE", type=strict_bool, default=True, help=f"true: fine-tune the encoder; false: optimise {latent} directly")
    p.add_argument("--independent", type=strict_bool, default=False,
                   help="true (with --optimizeE false): every image of a batch is an inversion of its own, equal to its batch-1 run")
    if launch:
        p.add_argument("--launch", choices=("eager", "graph"), default="graph")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--save_every", type=int, default=100)
    p.add_argument("--vgg_weights", default=None)
    p.add_argument("--lpips_weights", default=None)
    p.add_argument("--allow_standin_lpips", action="store_true")
    p.add_argument("--deterministic", action="store_true")


def make_parser():
    p = argparse.ArgumentParser(description="real-image inversion (embedding_v2_styleGAN1.py / embedding_v2_styleGAN2.py)")
    add_inversion_args(p, {}, 1, "./real_imgs/", "W+",
                       helps=dict(iterations="default: 1501 (mtype 1), 2001 (mtype 2)", lr="default 0.005", beta_1="default 0.0"))
    p.add_argument("--space", choices=("w", "z"), default="w",
                   help="with --optimizeE false: optimise the W+ code (w) or z in front of the mapping network (z; --mtype 1 or 2)")
    p.add_argument("--encoder", choices=ENCODERS, default="blur",
                   help="blur: E_Blur; be: E.BE, the encoder E_align trains (--checkpoint_dir_E then takes its checkpoints)")
    p.add_argument("--beta", type=float, default=None, help="weight of ||w1||_p: default 1e-3 (mtype 1), 3e-4 (mtype 2)")
    p.add_argument("--norm_p", type=int, default=None, help="p of ||w1||_p (default 2)")
    p.add_argument("--truncation", type=float, default=None, help="StyleGAN2: psi of avg + psi*(w1 - avg) (default 0.7; 1: none)")
    p.add_argument("--optimize_noise", type=strict_bool, default=False,
                   help="true (--mtype 2, --optimizeE false): optimise the synthesis network's noise maps beside the W+ code")
    p.add_argument("--noise_reg", type=float, default=1e5, help="weight of the noise regulariser in phase 1 (default 1e5)")
    p.add_argument("--noise_lr", type=float, default=None, help="learning rate of the noise maps (default: --lr)")
    return p


def parse_args(argv=None):
    """Parsed flags with the per-`--mtype` defaults filled in."""
    args = make_parser().parse_args(argv)
    if args.space == "z":
        if args.optimizeE:
            raise SystemExit("embedding_v2: --space z needs --optimizeE false (z is optimised against the frozen encoder)")
        if args.mtype not in (1, 2):
            raise SystemExit("embedding_v2: --space z is for --mtype 1 (StyleGAN1) or 2 (StyleGAN2); PGGAN and BigGAN optimise z already")
        if several_processes(env=True):
            raise SystemExit("embedding_v2: --space z runs in one process (WORLD_SIZE > 1 is not supported)")
    if args.mtype not in DEFAULTS:
        raise SystemExit("embedding_v2: --mtype must be 1 (StyleGAN1) or 2 (StyleGAN2)")
    if args.optimize_noise:
        why = noise_refusal(args.mtype == 2, args.optimizeE, args.space == "z", several_processes(env=True))
        if why:
            raise SystemExit("embedding_v2: --optimize_noise true: " + why)
    if args.independent and args.optimizeE:
        raise SystemExit("embedding_v2: --independent true needs --optimizeE false (the fine-tuned encoder is shared by a group)")
    for k, v in DEFAULTS[args.mtype].items():
        if getattr(args, k, None) is None:
            setattr(args, k, v)
    return args


IMAGE_EXT = (".png", ".jpg", ".jpeg", ".bmp")


def _load_imgs(path, size, device):
    if path.endswith(".pt"):
        return (torch.load(path, map_location="cpu").float() * 2 - 1).to(device)
    from .infer import load_images
    names = sorted(n for n in os.listdir(path) if n.lower().endswith(IMAGE_EXT))
    return load_images([os.path.join(path, n) for n in names], size, bicubic=True, device=device)


def open_run(args, LP, default_out, dev):
    """Behind the models of a CLI run: the LPIPS weights, the output tree (--experiment_dir) and the images -> (out, imgs)."""
    load_lpips_weights(LP, args.vgg_weights, args.lpips_weights, allow_standin=args.allow_standin_lpips)
    out = args.experiment_dir or default_out
    for sub in ("", "imgs", "models", "summaries"):
        os.makedirs(os.path.join(out, sub), exist_ok=True)
    return out, _load_imgs(args.img_dir, args.img_size, dev)


def run_inversion(args, st, invert, imgs, out, **walk_kw):
    """The tail of a CLI run: invert_folder over `imgs` with `invert` (invert_v2, invert_pg, invert_big) on the step `st`."""
    kw = dict(save_every=args.save_every, out_dir=out, **({"launch": args.launch} if "launch" in args else {}))
    invert_folder(lambda imgs1, **gk: invert(st, imgs1, args.iterations, **kw, **gk), imgs, args.batch_size, args.independent, out, **walk_kw)
    return st


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
    out, imgs = open_run(args, LP, "./realimg_embedding_result/7", dev)
    noise_kw = dict(optimize_noise=True, noise_reg=args.noise_reg, noise_lr=args.noise_lr) if args.optimize_noise else {}
    st = LatentEmbedStep(G, E, LP, mode="E" if args.optimizeE else ("Z" if zspace else "W"), Gm=Gm, generator="sg1" if args.mtype == 1 else "sg2", lr=args.lr,
                         beta_1=args.beta_1, beta=args.beta, norm_p=args.norm_p, truncation=args.truncation,
                         iterations=args.iterations, seed=args.seed, independent=args.independent, **noise_kw)
    return run_inversion(args, st, invert_v2, imgs, out, all_name="z_all_%d.pt" if zspace else "w_all_%d.pt")


if __name__ == "__main__":
    main()
