"""Mis-aligned encoder training on the HIP path: the iteration of `E_mis_align_cropping_s1.py` (reference
:109-206) and of the two Cat256 scripts `ablation_utils/Cat256/E_mis_align_case_1.py` (:109-206) and `E_mis_align_case_2.py`
(:110-214), with a command line (`python -m dge_amd.mis_align`).

What the shipped loops do, and what is kept.  All three: G -> E -> G as in E_align_s2; Grad-CAM++ masks of both image batches,
guided-back-propagation gradients, JET overlays (metric/grad_cam.py); image-space `space_loss` evaluations of gradients, images,
masks and overlays.

  s1     every image-space loss is built from detached tensors (:175-191), so `loss_tsa.backward()` reaches only LPIPS's own `lin`
         weights and the first `E_optimizer.step()` finds no gradient: the encoder is trained by the latent phase
         (`0.01 * loss_w`, :199-205) alone.  The second synthesis therefore runs without a gradient tape.  `loss_c` (:197, logged
         only) is not produced.
  case1  s1 with the latent phase `loss_mtv = (loss_c + loss_w) * 0.01`, `loss_c = space_loss(const1, const2, image_space=False)`:
         one backward carries g_w and g_const into the encoder's backward.  const1 is `Gs.const` repeated to the batch (mtype 1,
         :40-41) or `synthesis.early_layer.const` repeated to the batch (mtype 2, :61-62).
  case2  four optimizer calls per iteration (:172-214): (1) `space_loss(imgs1, imgs2)` on the full image, weight 1, with the
         gradient live through the second synthesis and E: zero_grad, backward(retain_graph), step; (2) `5 * space_loss(mask_1,
         mask_2)` and (3) `9 * space_loss(cam_1, cam_2)`: the masks and overlays are leaves in the script (numpy / cv2 products made
         tensors again, :182-197), no gradient reaches E, they are computed as values; (4) `loss_w` itself - NOT scaled by 0.01, the
         script's :213 back-propagates `loss_w` - zero_grad, backward, step.  `loss_c` (:207) and `loss_grad` (:172) are logged.

Decisions.
  * `zero_grad_to_none` (all cases; True = torch >= 2.0): an optimizer call whose loss reaches no encoder parameter - s1 / case1's
    image phase, case2's calls (2) and (3) - finds no gradient and does nothing.  False (`--legacy_zero_grad`; the torch < 2.0 of the
    reference's pinned environment zero-FILLS the gradients): each of them is `opt.tick()`, as EAlignStep's stage 1 does - every
    Adam state that exists advances its step counter and decays its second moment.  In case2 the two ticks sit between the image
    step and the latent step of every iteration, first iteration included.  In s1 / case1 the first such call of a run comes before
    any real step; the gradient tensors it finds are the ones the script's Grad-CAM backward through imgs2 left on the encoder
    (`_idle_call`), and they get their Adam state there (tests/golden/step_misalign_case1.npz, `legacy_` arrays: the first
    iteration already differs from the default form).
  * The attention pass has three routings with the same results: `separate` (the script's four passes), `fused` (one forward and
    one backward per image batch, GradCAM.with_input_gradient) and `pair` (both batches through VGG16 once,
    GradCAM.with_input_gradient_pair + mask2cam(groups=2): half the launches).  `fused_attention=True/False` keeps selecting the
    first two and stays the default of the class.
  * Refused, each with a message: case1 / case2 with mtype 3 or 4 (const1 is `tensor(0)` or the class vector there, :73 / :139:
    the script's loss_c is not meaningful); case1 when const1 and const2 differ in shape (the script's MSELoss refuses them; case2
    only logs loss_c and leaves `info_c` None then); `capture()` for case2 (a replayed graph of the four-call iteration has not been
    validated); `prefetch_next=True`; case1 / case2 in more than one process.
  * The script imports `model.E.E_Blur` in case 2 and `model.E.E` in case 1 / s1.  The iteration does not depend on which: the step
    takes the encoder it is given (an encoder_variants.BlurBE keeps its strided conv_2's forward-time data-gradient weights through
    the later backward, as e_align_case2 arranges); the command line builds E.BE, which the fixtures pin.
  * The command line runs eager launches in one process and writes the scripts' dumps (:284-309): every 100 iterations
    `imgs/ep%d_iter%d.png` (imgs1 over imgs2), `grad_cam/heatmap_%d.png`, `cam_%d.png`, `gb_%d.png` and a `Loss.txt` block, every
    5000 `models/E_model_ep%d_iter%d.pth`.  The guided-gradient picture is `grads -= np.max(np.min(grads), 0); grads /=
    np.max(grads)` in the script - the 0 is np.max's axis, so this is the global minimum and then the new maximum - done on the
    device (infer.minmax_unit) with no host read in front of the PNG.  No tensorboard scalars.
"""
import os

import torch

from . import losses, ops
from .e_align import EAlignStep
from .generators import generator_family
from .grad_cam import GradCamPlusPlus, GuidedBackPropagation, mask2cam
from .train_step import TrainStep

CASES = ("s1", "case1", "case2")
ATTENTION = ("pair", "fused", "separate")
MSG_MTYPE = ("MisAlignStep: case1 / case2 are offered for mtype 1 (StyleGAN1) and 2 (StyleGAN2): with PGGAN const1 is tensor(0) and with "
             "BigGAN the class vector, so the scripts' loss_c is not meaningful there")
MSG_CAPTURE = "MisAlignStep: hipGraph capture is not offered for case2 (four optimizer calls per iteration; eager launches only)"
MSG_PREFETCH = "MisAlignStep.step: prefetch_next is not offered (the generator pass opens its own iteration)"
MSG_DIST = "MisAlignStep: case1 / case2 run in a single process (the Cat256 scripts have no data-parallel form)"
MSG_PROCS = "mis_align: more than one process is not offered (eager launches, one process)"


class MisAlignStep(EAlignStep):
    def __init__(self, generator, E, lpips_model, vgg16, fused_attention=True, attention=None, case="s1", **kw):
        """`vgg16`: dge_amd.grad_cam.VGG16 (torchvision vgg16 layout), shared by Grad-CAM++ and guided back-propagation
        as in E_mis_align_cropping_s1.py:99-106.  `case`: "s1" | "case1" | "case2" and `zero_grad_to_none`: see the module docstring.
        `attention`: "pair" | "fused" | "separate"; None = "fused" / "separate" by `fused_attention`."""
        if case not in CASES:
            raise ValueError(f"MisAlignStep: case must be one of {CASES}, got {case!r}")
        if attention is None:
            attention = "fused" if fused_attention else "separate"
        if attention not in ATTENTION:
            raise ValueError(f"MisAlignStep: attention must be one of {ATTENTION}, got {attention!r}")
        if case != "s1" and generator_family(generator) in ("pggan", "biggan"):
            raise ValueError(MSG_MTYPE)
        super().__init__(generator, E, lpips_model, **kw)
        if case != "s1" and self.dist_on:
            raise RuntimeError(MSG_DIST)
        self.case, self.attention = case, attention
        self.grad_cam_plus_plus = GradCamPlusPlus(vgg16, vgg16.final_layer)
        self.gbp = GuidedBackPropagation(vgg16)
        self.fused_attention = attention != "separate"
        self.const1 = None
        if case == "case2":
            from .encoder_variants import BlurBE
            if isinstance(E, BlurBE):           # backward passes behind an optimizer step: see e_align_case2
                E.__dict__["_conv2_dgrad_at_forward"] = True

    _first_pass = TrainStep._first_pass          # the plain head: no prefetched pass, no early weight re-pack

    def capture(self, *a, **k):
        if self.case == "case2":
            raise RuntimeError(MSG_CAPTURE)
        return super().capture(*a, **k)

    def _const1(self):
        """:40-41 (mtype 1) / :61-62 (mtype 2: `early_layer(randn(batch))` is the learned constant repeated to the batch)"""
        if self.const1 is None or self.const1.shape[0] != self.batch_size:
            src = self.G.const if hasattr(self.gen, "Gm") else self.G.synthesis.early_layer.const
            self.const1 = src.detach().repeat(self.batch_size, 1, 1, 1).float().clone()
        return self.const1

    def _attention(self, imgs1, imgs2):
        """:159-170 -> mask_1, mask_2, grad_1, grad_2, heat_1, heat_2, cam_1, cam_2 (values)"""
        gcpp = self.grad_cam_plus_plus
        if self.attention == "pair":             # both batches through VGG16 once; the batch-coupled kernels in their group forms
            N = imgs1.shape[0]
            mask_1, grad_1, mask_2, grad_2 = gcpp.with_input_gradient_pair(imgs1, imgs2)
            heat, cam = mask2cam(gcpp.pair_mask, torch.cat((imgs1, imgs2)), groups=2)
            return mask_1, mask_2, grad_1, grad_2, heat[:N], heat[N:], cam[:N], cam[N:]
        if self.attention == "fused":            # one forward + one backward per batch instead of two of each (same results)
            mask_1, grad_1 = gcpp.with_input_gradient(imgs1)
            mask_2, grad_2 = gcpp.with_input_gradient(imgs2)
        else:
            mask_1 = gcpp(imgs1, None)
            mask_2 = gcpp(imgs2, None)
            grad_1 = self.gbp(imgs1)
            grad_2 = self.gbp(imgs2)
        heat_1, cam_1 = mask2cam(mask_1, imgs1)
        heat_2, cam_2 = mask2cam(mask_2, imgs2)
        return mask_1, mask_2, grad_1, grad_2, heat_1, heat_2, cam_1, cam_2

    def _idle_call(self, w2):
        """An optimizer call whose loss reached no encoder parameter: nothing (torch >= 2.0), or a step on zero-filled gradients.
        Zero-filled are the gradient tensors that exist: those of every parameter with optimizer state (`opt.tick()`) and, before
        the first real step of a run (s1 / case1, first iteration), those the script's Grad-CAM backward has already left behind -
        `grad_cam_plus_plus(imgs2, None)` back-propagates its class score through the synthesis into every encoder parameter that
        w2 depends on (:160).  LREQAdam gives these their state there: step 1, a second moment of zero, the value unchanged."""
        if self.zero_grad_to_none:
            return
        if any(len(st) for st in self.opt.state.values()):
            self.opt.tick()
            return
        params = [p for group in self.opt.param_groups for p in group["params"]]
        with torch.enable_grad():
            reached = torch.autograd.grad(w2.sum(), params, retain_graph=True, allow_unused=True)
        for p, g in zip(params, reached):
            if g is not None:
                self.opt.state[p]["step"] = 1
                self.opt.state[p]["exp_avg_sq"] = torch.zeros_like(p.data, memory_format=torch.contiguous_format)

    def step(self, iteration, z=None, noises=None, gen_noises=(None, None), new_z=None, prefetch_next=False):
        if prefetch_next:
            raise ValueError(MSG_PREFETCH)
        case2 = self.case == "case2"
        z, imgs1, w1, const2, w2, imgs2 = self._head(iteration, z, noises, gen_noises, new_z, synth_grad=case2)
        gctx = losses.GlobalBatch(self.world) if (self.dist_on and self.exact_ddp) else None         # (s1 only: see __init__)
        kw = dict(lpips_model=self.lpips, global_batch=gctx)
        phase = {}
        with torch.no_grad():
            imgs2_v = imgs2.detach()
            mask_1, mask_2, grad_1, grad_2, heat_1, heat_2, cam_1, cam_2 = self._attention(imgs1, imgs2_v)
            _, info_grad = losses.space_loss(grad_1, grad_2, **kw)
            if not case2:
                l_imgs, info_imgs = losses.space_loss(imgs1, imgs2_v, **kw)
        if case2:                                                    # (1) :175-179
            l_imgs, info_imgs = losses.space_loss(imgs1, imgs2, **kw)
            self.opt.zero_grad()
            l_imgs.backward(retain_graph=True)
            self.opt.step()
            phase["imgs"] = l_imgs = l_imgs.detach()
        with torch.no_grad():
            l_mask, info_mask = losses.space_loss(mask_1, mask_2, **kw)
            if case2:                                                # (2) :186-191
                phase["mask"] = l_mask * 5.0
                self._idle_call(w2)
            l_cam, info_cam = losses.space_loss(cam_1, cam_2, **kw)
            if case2:                                                # (3) :198-203
                phase["Gcam"] = l_cam * 9.0
            loss_tsa = l_imgs + l_mask + l_cam
            if not case2:
                phase["tsa"] = loss_tsa
            self._idle_call(w2)                                        # s1 / case1: the script's step on loss_tsa (:191-194)
        # latent phase
        c1 = self._const1() if self.case != "s1" else None
        loss_c = info_c = None
        if self.case == "case1":
            if c1.shape != const2.shape:
                raise ValueError(f"MisAlignStep case1: const1 {tuple(c1.shape)} and the encoder's const2 {tuple(const2.shape)} differ in "
                                 "shape: loss_c cannot be formed (the generator's and the encoder's widths must agree)")
            loss_c, info_c = losses.space_loss(c1, const2, image_space=False)
        elif case2 and c1.shape == const2.shape:
            with torch.no_grad():
                loss_c, info_c = losses.space_loss(c1, const2.detach(), image_space=False)
        loss_w, info_w = losses.space_loss(w1, w2, image_space=False, global_batch=gctx)
        loss_mtv = loss_w if case2 else (loss_w if loss_c is None else loss_c + loss_w) * 0.01
        self.opt.zero_grad()
        loss_mtv.backward()
        gs = self._sync_grads()
        self.opt.step(grad_scale=gs)
        ops.zero_arena_end()
        det = self.det
        phase["w" if case2 else "mtv"] = loss_mtv.detach()
        self.last = dict(imgs1=imgs1, imgs2=imgs2_v, w1=w1, w2=w2.detach(), const2=det(const2), mask_1=mask_1, mask_2=mask_2,
                         grad_1=grad_1, grad_2=grad_2, heatmap_1=heat_1, heatmap_2=heat_2, cam_1=cam_1, cam_2=cam_2,
                         loss_tsa=loss_tsa, info_imgs=info_imgs, info_mask=info_mask, info_Gcam=info_cam, info_grad=info_grad,
                         loss_w=loss_w.detach(), info_w=info_w, loss_c=det(loss_c), info_c=info_c, phase_losses=phase)
        return self.last


# ---------------------------------------------------------------------------------------------- command line
# (iterations, batch_size) of each script; --img_size 256 --start_features 64 --mtype 2 --lr 0.0015 --beta_1 0 in all three
CASE_DEFAULTS = {"s1": (210000, 5), "1": (120001, 8), "2": (120001, 8)}
_CASE_OF = {"s1": "s1", "1": "case1", "2": "case2"}


def _info_str(info):
    """the script's `loss_*_info` list: [[mse, mse of means, mse of stds], kl, cosine, ssim, lpips]"""
    if info is None:
        return "None"
    v = [float(x) for x in info.cpu().tolist()[1:]]
    return str([v[:3]] + v[3:])


def dump(out_dir, iteration, r, batch_size):
    """the script's every-100-iterations block (:284-307)"""
    from .infer import minmax_unit, save_image_grid
    ep, it = iteration // 30000, iteration % 30000
    n_row = batch_size
    save_image_grid(torch.cat((r["imgs1"][:n_row], r["imgs2"][:n_row])), os.path.join(out_dir, "imgs", "ep%d_iter%d.png" % (ep, it)), nrow=n_row)
    gb = minmax_unit(torch.cat((r["grad_1"], r["grad_2"])))             # on the device; the PNG writer makes the first host read
    for name, t in (("heatmap", torch.cat((r["heatmap_1"], r["heatmap_2"]))), ("cam", torch.cat((r["cam_1"], r["cam_2"]))), ("gb", gb)):
        # values in [0,1] (the script saves them as they are); save_image_grid takes [-1,1]
        save_image_grid(t * 2.0 - 1.0, os.path.join(out_dir, "grad_cam", "%s_%d.png" % (name, iteration)), nrow=n_row)
    with open(os.path.join(out_dir, "Loss.txt"), "a+") as f:
        print("i_" + str(iteration), file=f)
        print("[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]", file=f)
        print("---------ImageSpace--------", file=f)
        for key, tag in (("info_mask", "mask"), ("info_grad", "grad"), ("info_imgs", "imgs"), ("info_Gcam", "Gcam")):
            print("loss_%s_info: %s" % (tag, _info_str(r[key])), file=f)
        print("---------LatentSpace--------", file=f)
        print("loss_w_info: %s" % _info_str(r["info_w"]), file=f)
        print("loss_c_info: %s" % _info_str(r["info_c"]), file=f)


def train(tensor_writer=None, args=None, dump_every=100, save_every=5000):
    """The scripts' train().  `dump_every` / `save_every`: the periods of the picture + Loss.txt block and of the encoder checkpoint
    (the scripts' 100 and 5000; keywords so that a short run can see them)."""
    from .grad_cam import VGG16
    from .models import load_models, prepare_training
    G, Gm, E, LP = load_models(args)
    prepare_training(args, LP)
    vgg = VGG16(compute_dtype=getattr(args, "compute_dtype", "bf16")).to("cuda")
    if args.vgg16_weights:
        vgg.load_pretrained(args.vgg16_weights)
    else:
        print("mis_align: no --vgg16_weights: the attention maps come from a seeded stand-in VGG16 (NOT the reference's classifier)")
    st = MisAlignStep(G, E, LP, vgg, attention=args.attention, case=_CASE_OF[args.case], lr=args.lr, beta_1=args.beta_1,
                      batch_size=args.batch_size, z_dim=args.z_dim, mapping=Gm, zero_grad_to_none=not args.legacy_zero_grad)
    out_dir = args.experiment_dir
    if out_dir:
        for sub in ("", "imgs", "models", "grad_cam"):
            os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    for iteration in range(args.iterations):
        r = st.step(iteration)
        if iteration % dump_every == 0:
            print("ep_%d_iter_%d" % (iteration // 30000, iteration % 30000),
                  *["loss_%s %.6f" % (n, float(v)) for n, v in r["phase_losses"].items()])
            if out_dir:
                dump(out_dir, iteration, r, args.batch_size)
        if iteration % save_every == 0 and out_dir:
            torch.save(E.state_dict(), os.path.join(out_dir, "models", "E_model_ep%d_iter%d.pth" % (iteration // 30000, iteration % 30000)))
    return st


def build_parser(case="s1"):
    import argparse
    from .models import add_model_args, add_train_args
    iterations, batch = CASE_DEFAULTS[case]
    parser = argparse.ArgumentParser(description="the training args (mis-aligned encoder training)")
    parser.add_argument("--case", choices=tuple(CASE_DEFAULTS), default="s1", help="s1: E_mis_align_cropping_s1.py; 1 / 2: "
                        "ablation_utils/Cat256/E_mis_align_case_1.py / E_mis_align_case_2.py")
    add_train_args(parser, iterations=iterations)
    add_model_args(parser)
    parser.set_defaults(batch_size=batch, img_size=256, start_features=64, mtype=2)
    parser.add_argument("--legacy_zero_grad", action="store_true", help="optimizer.zero_grad() as torch < 2.0 (zero-filled gradients, the "
                        "reference's pinned environment): an optimizer call without a gradient ticks every Adam state")
    parser.add_argument("--vgg16_weights", default=None, help="torchvision vgg16 checkpoint for the attention maps (seeded stand-in without)")
    parser.add_argument("--attention", choices=ATTENTION, default="pair", help="pair: both image batches through VGG16 once; fused: one "
                        "forward and backward per batch; separate: the script's four passes (same results)")
    return parser


def parse_args(argv=None):
    import argparse
    import sys
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--case", default="s1")
    case = pre.parse_known_args(sys.argv[1:] if argv is None else argv)[0].case
    args = build_parser(case if case in CASE_DEFAULTS else "s1").parse_args(argv)       # (a bad --case is rejected by the full parser)
    if args.case != "s1" and args.mtype not in (1, 2):
        raise SystemExit("mis_align: " + MSG_MTYPE.split(": ", 1)[1])
    import torch.distributed as dist
    if (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1) or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(MSG_PROCS)
    return args


def main(argv=None):
    return train(None, parse_args(argv))


if __name__ == "__main__":
    main()
