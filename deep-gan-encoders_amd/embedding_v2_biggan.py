"""Real-image inversion of the reference's embedding_v2_BigGAN.py:25-230 on the HIP path: BigGAN-deep (BASELINE config 4's
generator) with the conditional-BN encoder E_BIG, in two modes:

  mode "E" (--optimizeE true):  the encoder is re-loaded per image group and fine-tuned; const1, w1 = E(imgs1, cond) every iteration.
  mode "W" (--optimizeE false): the encoder is frozen and the latent w1 [B,128] itself is optimised (LREQAdam on the leaf w1).

Once:      embed = G.embeddings(one_hot(label));  z0 = truncated_noise_sample(0.4, B, seed=iterations % 30000)
           cond_vector = cat(z0, embed)            (a constant: E's condition in every call)
Per group: [W] const1, w1 = E(imgs1, cond_vector) detached -> copied into the leaf w1, the Adam state cleared
           [E] the encoder checkpoint is re-loaded, the Adam state cleared          (embed_step.TwoPhaseEmbedStep.begin_image)
Per iteration:
    [E] const1, w1 = E(imgs1, cond_vector)
    imgs2, _ = G(w1, conditions, truncation);   const2, w2 = E(imgs2, cond_vector)
    loss_msiv = space_loss(imgs1, imgs2) [+ space_loss(mask_1, mask_2) + space_loss(cam_1, cam_2)]
    zero_grad; loss_msiv.backward(retain_graph=True); step
    loss_msLv = 0.01 * space_loss(w1, w2);  zero_grad; backward; step
    tracker: armed at iteration == iterations // 2, then a save whenever min > loss_msiv * 1.05

Decisions:
  * Phase 2.  w2 = E(imgs2) is evaluated before the phase-1 step, as the script does.  Phase 2 back-propagates through this
    iteration's graphs (E(imgs2) -> imgs2 -> G -> w1 [-> E(imgs1)]) with the live weights the phase-1 step left (the
    reference's `p.data` Adam update), and its direct term sees the updated w1, as in embedding_v2.LatentEmbedStep.  The image
    gradient of E(imgs2) is the E_BIG backward's need_img form (autograd_encbig, ops.affine_bwd_fromrgb_img).  loss_c2 =
    space_loss(const1, const2) is logged only.
  * Train mode.  G and E stay in train mode in both modes, as in the script (no .eval() anywhere): every forward runs one
    spectral-norm power iteration, E's conditional batch norms included.
  * Frozen W mode.  The E parameters are frozen (requires_grad_(False)); the encoder backward then runs with params=False: the data
    gradient alone.
  * Attention terms.  The script builds them from .detach().clone(): they are values.  They are computed under no_grad with
    grad_cam.GradCamPlusPlus and mask2cam, as mis_align.MisAlignStep does; GuidedBackPropagation is constructed on the shared
    network as in the script (:56-57: from then on every backward of that network is the guided one, the masks' too) but never
    called: the guided-backprop gradients and the heat maps the script also computes are unused and are not produced.
    attention=True is the default (it needs the vgg16 network); --attention false leaves the two terms out.
  * Tracker.  embed_track.EmbedTracker (the device-side dge_embed_track) with tracker_rules("sg1", iterations): armed at
    iterations // 2, hysteresis 1.05, no norm tracker, minima restart per group; the loop of a group is embedding_v2.invert_group
    (files through finish_group - the script's names - and dump_group), the folder walk of main() embedding_v2.invert_folder.
  * Not offered, each a ValueError / SystemExit with a clear message: capture() / hipGraph replay (the power iterations are
    host-sequenced; --mtype 4 is excluded from capture elsewhere too), independent=True on BigEmbedStep (the rows form is a class of
    its own, below), more than one process, and --beta / --norm_p (the norm term is commented out in the script, :163).
  * Independent rows (BigEmbedRowsStep, --independent true; mode W only).  The B rows of a group are B inversions of their own,
    each with its own class label (--labels): per-row losses (losses.space_loss_image_rows / space_loss_rows), per-row Grad-CAM++
    targets and mask2cam normalisation (GradCAM.call_per_image, mask2cam(rows=True)), one tracker per row.  Phase 1 back-propagates
    sum_b loss_msiv_b, phase 2 0.01 * sum_b space_loss_b(w1, w2); LREQAdam is element-wise, the batch norms use stored statistics.
      - z0 of the condition vector is the batch-1 draw, repeated for every row: a batch-1 run of any image draws exactly that.
      - Each forward of G and E runs ONE spectral-norm power iteration for the whole batch.  So row b equals the batch-1 run of
        image b started from the same weight_u / weight_v buffers - not the b-th run of a sequential loop, whose buffers the earlier
        images have advanced.
      - The encoder is shared by a group, so mode E has no rows form (ValueError); capture() / replay() and more than one process
        stay refused.
      - A short last group is padded by repeating its last image and label; the padded rows' outputs are dropped.
  * --optimizeE parses true / false strictly (the reference's `type=bool` cannot be switched off).
  * Without --config_dir the generator is BigGAN-deep-256 (BIGGAN_DEEP256, the released configuration).
"""
import argparse
import numbers
import os

import torch

from . import losses, ops
from .embed_step import TwoPhaseEmbedStep, several_processes
from .embedding_v2 import _refuse, add_inversion_args, invert_group, open_run, rows_plan, run_inversion, strict_bool  # noqa: F401 (rows_plan: re-exported)
from .generators import truncated_noise_sample

DEFAULTS = dict(iterations=1501, lr=0.0003, beta_1=0.0, batch_size=1, img_size=256, z_dim=128, start_features=64, label=30,
                truncation=0.4)
BIGGAN_DEEP256 = dict(output_dim=256, z_dim=128, class_embed_dim=128, channel_width=128, num_classes=1000,
                      layers=[[False, 16, 16], [True, 16, 16], [False, 16, 16], [True, 16, 8], [False, 8, 8], [True, 8, 8],
                              [False, 8, 8], [True, 8, 4], [False, 4, 4], [True, 4, 2], [False, 2, 2], [True, 2, 1]],
                      attention_layer_position=8, eps=1e-4, n_stats=51)

MSG_CAPTURE = ("BigEmbedStep: hipGraph capture / replay is not offered - every forward of G and E runs host-sequenced spectral-norm "
               "power iterations (train mode); run step()")
MSG_INDEPENDENT = ("BigEmbedStep: independent=True is not offered (the script couples the rows of a batch; run batch_size 1 per image) "
                   "- the rows form is BigEmbedRowsStep")
MSG_ROWS_MODE = "BigEmbedRowsStep: mode 'W' only - in mode 'E' one encoder is shared by the rows of a group"
MSG_DIST = "BigEmbedStep: more than one process is not offered (the inversion loop is a single-process loop)"
MSG_NORM = "embedding_v2_biggan: --beta / --norm_p are not offered (the norm term is commented out in embedding_v2_BigGAN.py:163)"
# dump names (embedding_v2.dump_group): the script names neither file by the loss (:203,218)
IMG_NAME, W_NAME = "id{n}_ep{i}-norm{norm:.2f}.jpg", "id{n}-i{k}-w{i}-norm{norm:f}.pt"


class BigEmbedStep(TwoPhaseEmbedStep):
    independent = False          # the rows form: BigEmbedRowsStep

    def __init__(self, G, E, lpips_model, mode="E", vgg16=None, attention=True, label=30, lr=0.0003, beta_1=0.0, truncation=0.4,
                 iterations=1501, arm_iter=None, events_cap=256, independent=False):
        """`vgg16`: dge_amd.grad_cam.VGG16 (torchvision vgg16 layout) for the attention terms; needed unless attention=False."""
        if independent:
            raise ValueError(MSG_INDEPENDENT)
        if several_processes():
            raise ValueError(MSG_DIST)
        if attention and vgg16 is None:
            raise ValueError("BigEmbedStep: attention=True needs the vgg16 network (dge_amd.grad_cam.VGG16); pass attention=False to "
                             "leave the attention terms out")
        # (tracker_rules("sg1"): armed at iterations // 2, the minima restart per group, embedding_v2_BigGAN.py:88)
        super().__init__(G, E, lpips_model, mode, "sg1", lr, beta_1, iterations, arm_iter, events_cap, type(self).independent)
        self.attention, self.label = bool(attention), int(label)
        self.truncation = torch.tensor(float(truncation), dtype=torch.float)      # float32 tensor, on the host (generators.BigGANAdapter)
        self.z_truncation = float(truncation)
        self._const1 = self.labels = self.conditions = self.cond_vector = None
        for p in G.parameters():
            p.requires_grad_(False)
        G.train(); E.train()                    # the script never leaves train mode
        if self.attention:
            from .grad_cam import GradCamPlusPlus, GuidedBackPropagation
            self.grad_cam_plus_plus = GradCamPlusPlus(vgg16, vgg16.final_layer)
            self.gbp = GuidedBackPropagation(vgg16)          # shared network: the masks' backward is the guided one, as in the script

    def capture(self, *a, **kw):
        raise ValueError(MSG_CAPTURE)

    replay = capture

    # ------------------------------------------------------------------ once per set of row labels
    def _setup(self, labels, dev):
        """embedding_v2_BigGAN.py:37-47: the class conditions of the rows (`labels`: one class id per row), their embeddings and the
        constant condition vector of the encoder; rebuilt when the labels (coupled form: their number) or the device change."""
        if self.cond_vector is not None and self.labels == labels and self.cond_vector.device == dev:
            return
        cfg, B = self.G.config, len(labels)
        self.labels = labels
        self.conditions = torch.zeros(B, cfg.num_classes, device=dev)
        self.conditions[torch.arange(B, device=dev), torch.tensor(labels, device=dev)] = 1.0
        with torch.no_grad():
            embed = ops.linear(self.conditions, self.G.embeddings.weight.detach())
        # rows form: the batch-1 draw for every row (rows 1.. of a batch-B draw are other numbers: no batch-1 run would see them)
        z0 = truncated_noise_sample(truncation=self.z_truncation, batch_size=1 if self.independent else B, dim_z=cfg.z_dim,
                                    seed=self.iterations % 30000)
        self.cond_vector = torch.cat((torch.tensor(z0, dtype=torch.float).to(dev).expand(B, -1), embed), dim=1).contiguous()

    # ------------------------------------------------------------------ per image group (begin_image: TwoPhaseEmbedStep)
    def _begin_group(self, imgs1):
        self._setup((self.label,) * imgs1.shape[0], imgs1.device)

    def _latent_shape(self, B):
        return (B, self.G.config.z_dim)

    def _start_code(self, imgs1, shape, noises, needed):
        """Mode W: const1, w1 = E(imgs1, cond_vector) - const1 stays as the logged constant, w1 is the start code unless `w_init` is
        given; the call runs either way (it advances the spectral-norm buffers)."""
        c0, w0 = self.E(imgs1, self.cond_vector, noises=noises)
        self._const1 = c0.detach().clone()
        return w0

    # ------------------------------------------------------------------ one iteration
    def _attention_terms(self, imgs1, imgs2):
        """space_loss(mask_1, mask_2) and space_loss(cam_1, cam_2) as values (:96-107,129-140).  Rows form: per row, every row's mask
        towards its own arg-max class and every cam normalised on its own."""
        from .grad_cam import mask2cam
        rows, cam = self.independent, self.grad_cam_plus_plus
        mask_of, image_loss = (cam.call_per_image, losses.space_loss_image_rows) if rows else (cam, losses.space_loss)
        with torch.no_grad():
            mask_1 = mask_of(imgs1.detach(), None)
            mask_2 = mask_of(imgs2.detach(), None)
            _, cam_1 = mask2cam(mask_1, imgs1, rows=rows)
            _, cam_2 = mask2cam(mask_2, imgs2, rows=rows)
            l_mask, info_mask = image_loss(mask_1, mask_2, lpips_model=self.lpips)
            l_cam, info_cam = image_loss(cam_1, cam_2, lpips_model=self.lpips)
        if rows:
            l_mask, l_cam = info_mask[:, 0].contiguous(), info_cam[:, 0].contiguous()
        return dict(mask_1=mask_1, mask_2=mask_2, cam_1=cam_1, cam_2=cam_2, loss_mask=l_mask, loss_Gcam=l_cam, info_mask=info_mask,
                    info_Gcam=info_cam)

    def step(self, imgs1, noises=(None, None)):
        """One iteration; `noises` = optional (E(imgs1), E(imgs2)) noise lists for parity runs (mode W: E(imgs1)'s is unused).  The
        attention terms are values (the script detaches them): they enter loss_msiv, not the gradient.  Rows form: an iteration of
        every row - phase 1 back-propagates sum_b space_loss_b(imgs1, imgs2), phase 2 0.01 * sum_b space_loss_b(w1, w2), and the
        logged values are the [B] columns of the info tensors."""
        E, rows = self.E, self.independent
        if self.group < 0:
            raise RuntimeError(f"{type(self).__name__}.step: call begin_image() first")
        image_loss, latent_loss = (losses.space_loss_image_rows, losses.space_loss_rows) if rows else (losses.space_loss, losses.space_loss)
        ops.zero_arena_begin(imgs1.device)
        if self.mode == "E":
            const1, w1 = E(imgs1, self.cond_vector, noises=noises[0])
        else:
            w1, const1 = self.w1, self._const1
        imgs2, _ = self.G(w1, self.conditions, self.truncation)
        const2, w2 = E(imgs2, self.cond_vector, noises=noises[1])
        loss_imgs, info_imgs = image_loss(imgs1, imgs2, lpips_model=self.lpips)
        if rows:          # the returned scalar is the sum over the rows: what phase 1 back-propagates
            loss_sum, loss_imgs = loss_imgs, info_imgs[:, 0].contiguous()
        loss_msiv, att = loss_imgs, {}
        if self.attention:
            att = self._attention_terms(imgs1, imgs2)
            loss_msiv = loss_imgs + att["loss_mask"] + att["loss_Gcam"]
        self._opt_phase(loss_sum if rows else loss_msiv, retain_graph=True)
        loss_w, info_w = latent_loss(w1, w2, image_space=False)
        with torch.no_grad():
            loss_c2, info_c2 = latent_loss(const1, const2, image_space=False)          # logged only
        loss_mslv = loss_w * 0.01
        self._opt_phase(loss_mslv)
        if rows:
            loss_w, loss_c2 = info_w[:, 0].contiguous(), info_c2[:, 0].contiguous()
            loss_mslv = loss_w * 0.01
        w1d = w1.detach()
        self._tracker.update(loss_msiv.detach(), w1d)
        ops.zero_arena_end()
        self.last = dict(w1=w1d, imgs2=imgs2.detach(), w2=w2.detach(), const1=const1.detach(), const2=const2.detach(),
                         loss_msiv=loss_msiv.detach(), loss_imgs=loss_imgs.detach(), info_imgs=info_imgs, loss_w=loss_w.detach(),
                         info_w=info_w, loss_c2=loss_c2.detach(), info_c2=info_c2, loss_mslv=loss_mslv.detach(),
                         w_norm=self._tracker.l2, **att)
        return self.last


class BigEmbedRowsStep(BigEmbedStep):
    """BigEmbedStep with the B rows of a group as B inversions of their own (mode W), each with its own class label.

    Row b equals the batch-1 BigEmbedStep run of image b with label b STARTED FROM THE SAME weight_u / weight_v BUFFERS: each forward
    of G and E runs one spectral-norm power iteration for the whole batch.  It does not equal the b-th run of a sequential loop,
    whose buffers the earlier images have advanced.  The logged values of step() (`loss_msiv`, `loss_imgs`, `loss_w`, `loss_c2`,
    `loss_mslv`, `w_norm`, the attention losses) are [B] columns, the infos [B,8]; tracker() returns one read-out per row."""
    independent = True

    def __init__(self, G, E, lpips_model, mode="W", **kw):
        if mode != "W":
            raise ValueError(MSG_ROWS_MODE)
        if kw.pop("independent", True) is not True:
            raise ValueError("BigEmbedRowsStep is the independent form; the coupled loop is BigEmbedStep")
        super().__init__(G, E, lpips_model, mode="W", **kw)

    def _row_labels(self, labels, B):
        if labels is None:
            labels = self.label
        if isinstance(labels, numbers.Integral) or (torch.is_tensor(labels) and labels.dim() == 0):
            labels = [int(labels)] * B
        labels = [int(v) for v in labels]
        K = self.G.config.num_classes
        if len(labels) != B:
            raise ValueError(f"BigEmbedRowsStep: {len(labels)} labels for {B} images")
        if any(v < 0 or v >= K for v in labels):
            raise ValueError(f"BigEmbedRowsStep: class ids must lie in [0, {K}), got {labels}")
        return tuple(labels)

    def _begin_group(self, imgs1, labels=None):
        """`labels` of begin_image: an int or one class id per row (default: the constructor's `label`) - the rows' conditions."""
        self._setup(self._row_labels(labels, imgs1.shape[0]), imgs1.device)


def invert_big(st, imgs1, iterations, save_every=100, out_dir=None, group=0, labels=None, keep=None):
    """`iterations` iterations on one image group (eager: there is no captured form).  With `out_dir` the script's
    every-`save_every` dumps (image pair, per-row w1, Loss.txt: one host read per dump) and, at the end, the tracker's files.
    Returns the last result dict with the tracker read-out under "tracker".  Rows form (BigEmbedRowsStep; `labels`: one class id per
    row): files carry the image number group * B + b, Loss.txt gets a block per image, only the first `keep` rows (default: all) are
    written, and "tracker" is the list of per-row read-outs."""
    if not st.independent and (labels is not None or keep is not None):
        raise ValueError("invert_big: labels / keep belong to the rows form (BigEmbedRowsStep)")
    return invert_group(st, imgs1, iterations, "eager", save_every, out_dir, group, keep, dict(labels=labels) if st.independent else {},
                        dict(img_name=IMG_NAME, w_name=W_NAME, loss_txt=True))


def build_models_big_v2(config=None, img_size=256, start_features=64, compute_dtype="bf16", device="cuda", seed=0, attention=True):
    """BigGAN-deep (`config`: a BigGANConfig, default BigGAN-deep-256) + E_BIG + LPIPS through models.build_models_big, and the vgg16
    network of the attention terms (None without them).  Seeded random-init weights."""
    from .biggan_generator import BigGANConfig
    from .models import build_models_big
    G, E, LP = build_models_big(config or BigGANConfig.from_dict(BIGGAN_DEEP256), img_size, start_features, compute_dtype, device=device,
                                seed=seed)
    vgg = None
    if attention:
        from .grad_cam import VGG16
        vgg = VGG16(compute_dtype=compute_dtype).to(device)
    return G, E, LP, vgg


# ------------------------------------------------------------------ CLI
def make_parser():
    p = argparse.ArgumentParser(description="BigGAN-deep real-image inversion (embedding_v2_BigGAN.py)")
    add_inversion_args(p, DEFAULTS, 4, "./bigGAN_inversion/id30/", "the latent", launch=False)
    p.set_defaults(img_size=DEFAULTS["img_size"], z_dim=DEFAULTS["z_dim"], start_features=DEFAULTS["start_features"])
    p.add_argument("--attention", type=strict_bool, default=True, help="false: leave the Grad-CAM++ mask / cam terms out of loss_msiv")
    p.add_argument("--label", type=int, default=DEFAULTS["label"], help="ImageNet class id of the condition (30: frog)")
    p.add_argument("--labels", default=None, help="with --independent true: one class id per image in the sorted order of --img_dir, "
                                                  "as a comma list or a text file with one id per line (default: --label for all)")
    p.add_argument("--truncation", type=float, default=DEFAULTS["truncation"])
    p.add_argument("--beta", type=_refuse(MSG_NORM), default=None, help="not offered: the norm term is commented out in the script")
    p.add_argument("--norm_p", type=_refuse(MSG_NORM), default=None, help="not offered: the norm term is commented out in the script")
    p.add_argument("--vgg16_weights", default=None, help="torchvision vgg16 checkpoint for the attention terms (seeded stand-in without)")
    return p


def parse_args(argv=None):
    args = make_parser().parse_args(argv)
    if args.mtype != 4:
        raise SystemExit("embedding_v2_biggan: --mtype is 4 (BigGAN-deep + E_BIG); the StyleGAN loops are dge_amd.embedding_v2")
    if args.independent and args.optimizeE:
        raise SystemExit("embedding_v2_biggan: --independent true needs --optimizeE false (the fine-tuned encoder is shared by a group)")
    if args.labels is not None and not args.independent:
        raise SystemExit("embedding_v2_biggan: --labels needs --independent true (the coupled loop has one --label for the batch)")
    return args


def read_labels(spec, n_images, num_classes, default):
    """The class id of every image: `spec` None -> `default` for all; a comma list, or the path of a text file with one id per line.
    A wrong count or an id outside [0, num_classes) is a SystemExit."""
    if spec is None:
        return [int(default)] * n_images
    try:
        if os.path.isfile(spec):
            with open(spec) as f:
                ids = [int(tok) for tok in f.read().split()]
        else:
            ids = [int(tok) for tok in spec.split(",") if tok.strip()]
    except ValueError:
        raise SystemExit(f"embedding_v2_biggan: --labels holds integer class ids (a comma list or a text file), got {spec!r}")
    if len(ids) != n_images:
        raise SystemExit(f"embedding_v2_biggan: --labels names {len(ids)} class ids for {n_images} images")
    bad = [v for v in ids if v < 0 or v >= num_classes]
    if bad:
        raise SystemExit(f"embedding_v2_biggan: --labels: class ids {bad} lie outside [0, {num_classes})")
    return ids


def main(argv=None):
    args = parse_args(argv)
    if args.deterministic:
        ops.set_deterministic(True)
    from .biggan_generator import BigGANConfig
    dev = "cuda"
    config = BigGANConfig.from_json_file(args.config_dir) if args.config_dir else None
    G, E, LP, vgg = build_models_big_v2(config, args.img_size, args.start_features, args.compute_dtype, device=dev, seed=args.seed,
                                        attention=args.attention)
    # the mtype-4 containers of models.load_models: the generator a bare state_dict, the encoder a bare state_dict
    if args.checkpoint_dir_GAN:
        G.load_state_dict(torch.load(args.checkpoint_dir_GAN, map_location="cpu"))
    if args.checkpoint_dir_E:
        E.load_state_dict(torch.load(args.checkpoint_dir_E, map_location="cpu"))
    if vgg is not None and args.vgg16_weights:
        vgg.load_pretrained(args.vgg16_weights)
    out, imgs = open_run(args, LP, "./result_bigGAN_id30_GradCAM/mis_aligh_bigGAN_v1_opE", dev)
    kw = dict(vgg16=vgg, attention=args.attention, label=args.label, lr=args.lr, beta_1=args.beta_1, truncation=args.truncation,
              iterations=args.iterations)
    labels = None
    if args.independent:
        labels = read_labels(args.labels, imgs.shape[0], G.config.num_classes, args.label)
        st = BigEmbedRowsStep(G, E, LP, **kw)
    else:
        st = BigEmbedStep(G, E, LP, mode="E" if args.optimizeE else "W", **kw)
    return run_inversion(args, st, invert_big, imgs, out, labels=labels, save_imgs=True)


if __name__ == "__main__":
    main()
