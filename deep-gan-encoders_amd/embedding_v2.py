"""Real-image inversion of the reference's v2 scripts (embedding_v2_styleGAN1.py:71-189, embedding_v2_styleGAN2.py:82-210) on the
HIP path, for StyleGAN1 (`--mtype 1`: Gs + E_Blur) and StyleGAN2 (`--mtype 2`: StyleGAN2 synthesis + E_Blur), in two modes
(`--encoder be` puts E.BE, the encoder E_align trains, in E_Blur's place):

  mode "E" (--optimizeE true):  the encoder is re-loaded per image group and fine-tuned; w1 = E(imgs1) every iteration.
  mode "W" (--optimizeE false): the encoder is frozen and the W+ code w1 itself is optimised (LREQAdam on the leaf w1).

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
  * Trackers are device-side (dge_embed_track): the device keeps the latest best latent of each kind and a bounded event log
    (iteration, kind, loss, norm); the host writes the final best .pt per kind with the reference's file names and
    loss_min.txt from the log at the end of each group.
  * W mode takes a batch B >= 1 (the reference hard-codes 1); the norm and space_loss terms couple the rows as in the reference.
    StyleGAN2's W-mode start is randn(B, L, 512) from a seeded generator (unseeded in the reference).
  * --optimizeE parses true / false strictly (the reference's `type=bool` cannot be switched off).
  * `independent` (--independent true; W mode only): the B rows of a group are B inversions of their own, each equal to the
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
"""
import argparse
import math
import os

import torch

from . import losses, ops, weight_cache
from .custom_adam import LREQAdam
from .embedding import select_launch
from .graph_step import GraphReplay
from .models import add_model_args, blur_encoder, load_lpips_weights

# per-generator defaults (embedding_v2_styleGAN1.py:195-209 + :118,128-131; embedding_v2_styleGAN2.py:214-232 + :136,153-166)
DEFAULTS = {
    1: dict(iterations=1501, lr=0.005, beta_1=0.0, beta=1e-3, norm_p=2, truncation=None),
    2: dict(iterations=2001, lr=0.005, beta_1=0.0, beta=3e-4, norm_p=2, truncation=0.7),
}
IMG_WEIGHTS = (1.0, 0.125 * 3, 0.125 * 5)
EVENT_LOSS, EVENT_NORM = 0, 1


def tracker_rules(generator, iterations):
    """The reference's best-loss / best-norm `if` chains as parameters of dge_embed_track."""
    if generator == "sg1":        # armed at iterations//2 (min := that loss), hysteresis 1.05, no norm tracker, reset per group
        return dict(arm_rule=ops.TRACK_ARM_AT, arm_iter=iterations // 2, loss_hyst=1.05, norm_hyst=0.0, init=(0.0, 0.0),
                    reset_per_group=True)
    # iteration > 1000, hysteresis 1.03 / 1.05, minima start at 100 / 1000 and carry over between groups
    return dict(arm_rule=ops.TRACK_ARM_AFTER, arm_iter=1000, loss_hyst=1.03, norm_hyst=1.05, init=(100.0, 1000.0),
                reset_per_group=False)


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
    def __init__(self, G, E, lpips_model, mode="E", generator="sg2", lr=0.005, beta_1=0.0, beta=None, norm_p=2, truncation=None,
                 iterations=None, arm_iter=None, events_cap=256, seed=0, independent=False):
        if mode not in ("E", "W"):
            raise ValueError(f"mode must be 'E' or 'W', got {mode!r}")
        if independent and mode != "W":
            raise ValueError("independent=True needs mode 'W': in mode 'E' one encoder is shared by the rows of a group")
        self.independent = bool(independent)
        if generator not in ("sg1", "sg2"):
            raise ValueError(f"generator must be 'sg1' or 'sg2', got {generator!r}")
        mt = 1 if generator == "sg1" else 2
        d = DEFAULTS[mt]
        self.G, self.E, self.lpips = G, E, lpips_model
        self.mode, self.generator = mode, generator
        self.lr, self.beta_1 = lr, beta_1
        self.beta = d["beta"] if beta is None else float(beta)
        self.norm_p = int(norm_p)
        self.psi = (d["truncation"] if truncation is None else float(truncation)) if generator == "sg2" else None
        self.iterations = d["iterations"] if iterations is None else int(iterations)
        self.rules = tracker_rules(generator, self.iterations)
        if arm_iter is not None:
            self.rules["arm_iter"] = int(arm_iter)
        self.events_cap, self.seed = int(events_cap), seed
        self.lod = G.layer_count - 1 if generator == "sg1" else None
        self.group = -1
        self.last = {}
        self.w1 = self._const2 = None
        self._track = None
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

    def _track_alloc(self, shape, dev):
        n = int(math.prod(shape))
        t = self._track
        if self.independent:      # a tracker per row: every state array gets a leading batch dimension
            B = shape[0]
            if t is None or t["n"] != n or t["fstate"].device != torch.device(dev):
                self._track = t = dict(n=n, istate=torch.zeros((B, 4), dtype=torch.int32, device=dev),
                                       fstate=torch.tensor([self.rules["init"]] * B, dtype=torch.float32, device=dev),
                                       best_loss=torch.zeros(shape, dtype=torch.float32, device=dev),
                                       best_norm=torch.zeros(shape, dtype=torch.float32, device=dev),
                                       events=torch.zeros((B, self.events_cap, 4), dtype=torch.float32, device=dev),
                                       l2=torch.zeros(B, dtype=torch.float32, device=dev))
            return t
        if t is None or t["n"] != n or t["fstate"].device != torch.device(dev):
            self._track = t = dict(n=n, istate=torch.zeros(4, dtype=torch.int32, device=dev),
                                   fstate=torch.tensor(self.rules["init"], dtype=torch.float32, device=dev),
                                   best_loss=torch.zeros(shape, dtype=torch.float32, device=dev),
                                   best_norm=torch.zeros(shape, dtype=torch.float32, device=dev),
                                   events=torch.zeros((self.events_cap, 4), dtype=torch.float32, device=dev),
                                   l2=torch.zeros((), dtype=torch.float32, device=dev))
        return t

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
        shape = (B, self._num_rows(), 512)
        if self.mode == "E":
            self.E.load_state_dict(self._ckpt)
            weight_cache.written(self.E.parameters())
            self._reset_opt()
        else:
            with torch.no_grad():
                if w_init is not None:
                    w0 = w_init.to(dev, torch.float32).reshape(shape)
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
                        raise ValueError("LatentEmbedStep.begin_image: the captured iteration works on a different W+ shape")
                    self.w1 = torch.zeros(shape, dtype=torch.float32, device=dev, requires_grad=True)
                    self.opt = LREQAdam([{"params": [self.w1]}], lr=self.lr, betas=(self.beta_1, 0.99), weight_decay=0)
                self.w1.copy_(w0)
            self._reset_opt()
        t = self._track_alloc(shape, dev)
        first = getattr(self, "_track_started", False) is False
        t["istate"].zero_()
        t["events"].zero_()
        if first or self.rules["reset_per_group"] or self.independent:
            t["fstate"].copy_(torch.tensor(self.rules["init"], dtype=torch.float32).expand_as(t["fstate"]))
        self._track_started = True

    # ------------------------------------------------------------------ one iteration
    def _generate(self, w1, noises):
        if self.generator == "sg1":
            return self.G.forward(w1, self.lod, noises=noises)
        syn = self.G.synthesis
        # (the synthesis backward reads its saved activations only, never wp: w1 itself may be the input when psi == 1)
        wt = w1 if self.psi == 1.0 else _WplusLerp.apply(w1, self.G.truncation.w_avg, self.psi)
        return syn(wt, randomize_noise=False)["image"]

    def step(self, imgs1, noises=(None, None, None)):
        """One iteration; `noises` = optional (E(imgs1), G, E(imgs2)) noise lists for parity runs (StyleGAN2: G's is unused, the
        synthesis noise is its fixed buffers; W mode: E(imgs1)'s is unused).  Independent mode: the loss entries of the result
        (`loss_msiv`, `loss_w`, `loss_c1`, `norm`, `loss_mslv`, `w_norm`) are [B], `info_img` is [B,3,8]."""
        E = self.E
        rows = self.independent
        t = self._track
        if t is None:
            raise RuntimeError("LatentEmbedStep.step: call begin_image() first")
        ops.zero_arena_begin(imgs1.device)
        if self.mode == "E":
            const2, w1 = E(imgs1, noises=noises[0])
        else:
            w1, const2 = self.w1, self._const2
        imgs2 = self._generate(w1, noises[1])
        if self.generator == "sg1":
            const3, w2 = E(imgs2, noises=noises[2])
        image_loss, latent_loss = (losses.image_loss_tsa_rows, losses.space_loss_rows) if rows else (losses.image_loss_tsa, losses.space_loss)
        loss_msiv, info_img = image_loss(imgs1, imgs2, self.lpips, weights=IMG_WEIGHTS, grad_windows=(True, True, True))
        self.opt.zero_grad()
        loss_msiv.backward(retain_graph=True)
        self.opt.step()
        if self.generator == "sg2":
            const3, w2 = E(imgs2, noises=noises[2])
        loss_w, info_w = latent_loss(w1, w2, image_space=False)
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
        r = self.rules
        if rows:      # the values of every row: the [B] columns of the info tensors (the scalars above are their sums over the rows)
            loss_msiv = info_img[:, 0, 0] * IMG_WEIGHTS[0] + info_img[:, 1, 0] * IMG_WEIGHTS[1] + info_img[:, 2, 0] * IMG_WEIGHTS[2]
            loss_w = info_w[:, 0].contiguous()
            loss_mslv = loss_w * 0.01 + nrm.detach() * self.beta
            if loss_c1 is not None:
                loss_c1 = info_c[:, 0].contiguous()
                loss_mslv = loss_mslv + loss_c1 * 0.01
            ops.latent_l2_rows(w1d, out=t["l2"])
            ops.embed_track_rows(loss_msiv, t["l2"], w1d, t["istate"], t["fstate"], t["best_loss"], t["best_norm"], t["events"],
                                 r["arm_rule"], r["arm_iter"], r["loss_hyst"], r["norm_hyst"])
        else:
            ops.latent_l2(w1d, out=t["l2"])
            ops.embed_track(loss_msiv.detach(), t["l2"], w1d, t["istate"], t["fstate"], t["best_loss"], t["best_norm"], t["events"],
                            r["arm_rule"], r["arm_iter"], r["loss_hyst"], r["norm_hyst"])
        ops.zero_arena_end()
        self.last = dict(w1=w1d, imgs2=imgs2.detach(), w2=w2.detach(), const2=const2.detach() if const2 is not None else None,
                         const3=const3.detach(), loss_msiv=loss_msiv.detach(), info_img=info_img, loss_w=loss_w.detach(),
                         loss_c1=loss_c1.detach() if loss_c1 is not None else None, norm=nrm.detach(), loss_mslv=loss_mslv.detach(),
                         w_norm=t["l2"])
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
        t = self._track
        if self.independent:
            B, cap = t["istate"].shape[0], self.events_cap
            # one host read: the three small state arrays travel as one float tensor (counters < 2^24 are exact in f32)
            host = torch.cat((t["istate"].float(), t["fstate"], t["events"].reshape(B, -1)), dim=1).cpu()
            bl, bn = t["best_loss"], t["best_norm"]
            out = []
            for b in range(B):
                ist = [int(v) for v in host[b, :4]]
                ev = host[b, 6:].view(cap, 4)
                idx = [k % cap for k in range(max(0, ist[1] - cap), ist[1])]
                out.append(dict(iteration=ist[0], events=[(int(ev[i, 0]), int(ev[i, 1]), float(ev[i, 2]), float(ev[i, 3])) for i in idx],
                                dropped=ist[2], min_loss=float(host[b, 4]), min_norm=float(host[b, 5]), best_loss=bl[b:b + 1].clone(), best_norm=bn[b:b + 1].clone()))
            return out
        ist = t["istate"].cpu().tolist()
        cnt, cap = ist[1], self.events_cap
        ev = t["events"].cpu()
        idx = [k % cap for k in range(max(0, cnt - cap), cnt)]
        events = [(int(ev[i, 0]), int(ev[i, 1]), float(ev[i, 2]), float(ev[i, 3])) for i in idx]
        return dict(iteration=ist[0], events=events, dropped=ist[2], min_loss=float(t["fstate"][0]), min_norm=float(t["fstate"][1]),
                    best_loss=t["best_loss"].clone(), best_norm=t["best_norm"].clone())


def write_tracker_files(tr, g, models_dir, result_dir):
    """The reference's outputs of the trackers for group g: the final best latent per kind (file names of
    embedding_v2_styleGAN2.py:156,163) and loss_min.txt lines (:159,166) from the event log."""
    last = {}
    loss_min = None
    with open(os.path.join(result_dir, "loss_min.txt"), "a+") as f:
        for it, kind, loss, norm in tr["events"]:
            if kind == EVENT_LOSS:
                loss_min = loss
                print("ep%d_iter%d_minImg%.5f_wNorm%f" % (g, it, loss, norm), file=f)
            else:
                print("ep%d_iter%d_Img%.5f_wNorm-min%f" % (g, it, loss, norm), file=f)
            last[kind] = (it, loss, norm, loss_min)
    if EVENT_LOSS in last:
        it, loss, norm, _ = last[EVENT_LOSS]
        torch.save(tr["best_loss"], os.path.join(models_dir, "id%d-iter%d-norm%f-imgLoss-min%f.pt" % (g, it, norm, loss)))
    if EVENT_NORM in last:
        it, loss, norm, lm = last[EVENT_NORM]
        torch.save(tr["best_norm"], os.path.join(models_dir, "id%d-iter%d-norm-min%f-imgLoss%f.pt" % (g, it, norm, lm if lm is not None else 0.0)))


def group_plan(n_images, batch_size):
    """Independent mode: the groups of a folder of n_images as (first image number, rows kept) - every image is inverted, the last
    group may keep fewer rows than the batch holds."""
    return [(i, min(batch_size, n_images - i)) for i in range(0, n_images, batch_size)]


def padded_rows(first, batch_size, n_images):
    """Image numbers of the batch_size rows of the group that starts at image `first`: a short last group repeats its last image
    (the captured iteration keeps its shape); the caller discards those rows' outputs."""
    return [min(first + r, n_images - 1) for r in range(batch_size)]


def invert_v2(st, imgs1, iterations, launch="graph", save_every=100, out_dir=None, group=0, w_init=None, keep=None):
    """`iterations` iterations on one image group.  launch="graph" captures the iteration once (its warm-up iteration is a real one)
    and replays it; later groups go through set_image.  With `out_dir` the reference's every-`save_every` dumps (image pair,
    per-row w1) are written - one host read per chunk - and, at the end, the trackers' files.  Returns the last result dict with
    the tracker read-out under "tracker".  Independent mode: files carry the image number group*B + b and that row's norm and loss;
    only the first `keep` rows (default: all) are written, and "tracker" is the list of per-row read-outs."""
    st.begin_image(imgs1, w_init=w_init)
    if launch not in ("graph", "eager"):
        raise ValueError(f"launch must be 'graph' or 'eager', got {launch!r}")
    run, done = select_launch(st, imgs1, launch)
    r = st.last

    def dump(i, r):
        if out_dir is None:
            return
        from .infer import save_image_grid
        B = imgs1.shape[0]
        if st.independent:
            vals = torch.stack((r["w_norm"], r["loss_msiv"])).cpu()
            for b in range(B if keep is None else keep):
                num, norm, loss = group * B + b, float(vals[0, b]), float(vals[1, b])
                save_image_grid(torch.cat((imgs1[b:b + 1], r["imgs2"][b:b + 1])), os.path.join(out_dir, "imgs", "id%d_ep%d-norm%.2f-imgLoss%f.jpg"
                                                                                              % (num, i, norm, loss)), nrow=2)
                torch.save(r["w1"][b:b + 1].clone().cpu(), os.path.join(out_dir, "models", "id%d-i%d-w%d-norm%f-imgLoss%f.pt"
                                                                        % (num, 0, i, norm, loss)))
            return
        norm, loss = float(r["w_norm"]), float(r["loss_msiv"])
        save_image_grid(torch.cat((imgs1[:B], r["imgs2"][:B])), os.path.join(out_dir, "imgs", "id%d_ep%d-norm%.2f-imgLoss%f.jpg"
                                                                            % (group, i, norm, loss)), nrow=2)
        for k, row in enumerate(r["w1"]):
            torch.save(row.unsqueeze(0).clone().cpu(), os.path.join(out_dir, "models", "id%d-i%d-w%d-norm%f-imgLoss%f.pt"
                                                                     % (group, k, i, norm, loss)))

    if done and save_every:
        dump(0, r)                              # iteration 0 ran as capture()'s warm-up
    for i in range(done, iterations):
        r = run()
        if save_every and i % save_every == 0:
            dump(i, r)
    tr = st.tracker()
    if out_dir is not None and st.independent:
        for b in range(imgs1.shape[0] if keep is None else keep):
            write_tracker_files(tr[b], group * imgs1.shape[0] + b, os.path.join(out_dir, "models"), out_dir)
    elif out_dir is not None:
        write_tracker_files(tr, group, os.path.join(out_dir, "models"), out_dir)
    r = dict(r)
    r["tracker"] = tr
    return r


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


def load_checkpoints(G, E, mtype, gan=None, enc=None):
    """The checkpoint containers of models.load_models: mtype 2 a dict holding `generator_smooth` (or `generator`), mtype 1 a
    directory with Gs_dict.pth; the encoder a bare state_dict."""
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
    from .infer import save_image_grid
    dev = "cuda"
    G, E, LP = build_models_v2(args.mtype, args.img_size, args.start_features, args.compute_dtype, device=dev, seed=args.seed,
                               fmaps_base=args.fmaps_base, fmaps_max=args.fmaps_max, enc_maxf=args.enc_maxf, encoder=args.encoder)
    load_checkpoints(G, E, args.mtype, args.checkpoint_dir_GAN, args.checkpoint_dir_E)
    load_lpips_weights(LP, args.vgg_weights, args.lpips_weights, allow_standin=args.allow_standin_lpips)
    out = args.experiment_dir or "./realimg_embedding_result/7"
    for sub in ("", "imgs", "models", "summaries"):
        os.makedirs(os.path.join(out, sub), exist_ok=True)
    imgs = _load_imgs(args.img_dir, args.img_size, dev)
    st = LatentEmbedStep(G, E, LP, mode="E" if args.optimizeE else "W", generator="sg1" if args.mtype == 1 else "sg2", lr=args.lr,
                         beta_1=args.beta_1, beta=args.beta, norm_p=args.norm_p, truncation=args.truncation,
                         iterations=args.iterations, seed=args.seed, independent=args.independent)
    bs = args.batch_size
    w_all = []
    if args.independent:
        n = imgs.shape[0]
        for g, (first, keep) in enumerate(group_plan(n, bs)):
            imgs1 = imgs[padded_rows(first, bs, n)].contiguous()
            r = invert_v2(st, imgs1, args.iterations, launch=args.launch, save_every=args.save_every, out_dir=out, group=g, keep=keep)
            vals = torch.stack((r["loss_msiv"], r["w_norm"])).cpu()
            for b in range(keep):
                print("image %d: loss_msiv %.5f  w_norm %.4f  events %d" % (first + b, float(vals[0, b]), float(vals[1, b]),
                                                                          len(r["tracker"][b]["events"])))
                w_all.append(r["w1"][b].clone().cpu())
            save_image_grid(r["imgs2"][:keep], os.path.join(out, "summaries", "%s_rec.png" % str(g).rjust(5, "0")), nrow=bs)
        if w_all:
            torch.save(torch.stack(w_all, dim=0), os.path.join(out, "models", "w_all_%d.pt" % (n - 1)))
        return st
    ngroups = imgs.shape[0] // bs
    for g in range(ngroups):
        imgs1 = imgs[g * bs:(g + 1) * bs].contiguous()
        r = invert_v2(st, imgs1, args.iterations, launch=args.launch, save_every=args.save_every, out_dir=out, group=g)
        print("group %d: loss_msiv %.5f  w_norm %.4f  events %d" % (g, float(r["loss_msiv"]), float(r["w_norm"]), len(r["tracker"]["events"])))
        save_image_grid(r["imgs2"], os.path.join(out, "summaries", "%s_rec.png" % str(g).rjust(5, "0")), nrow=bs)
        w_all.append(r["w1"][0].clone().cpu())
    if w_all:
        torch.save(torch.stack(w_all, dim=0), os.path.join(out, "models", "w_all_%d.pt" % (ngroups - 1)))
    return st


if __name__ == "__main__":
    main()
