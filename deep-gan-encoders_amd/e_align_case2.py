"""Per-loss-update encoder training ("case 2") with the E_Blur encoder on the HIP path: the ablation ladder
ablation_utils/4.E_align_w_zn.py .. 8.E_align_x_AT1_AT2.py (StyleGAN1) and ablation_utils/Cat256/E_align_case_2.py (StyleGAN2).

Case 1 (dge_amd.e_align) makes one optimizer step on loss_imgs + 5*AT1 + 9*AT2 and one on the latent loss.  Case 2 - the
configuration behind the paper's better numbers (E_align_case_2.py:180-182) - uses E_Blur, detaches nothing and updates
"different vectors separately": one iteration of script 8 (`Case2Step.step`, 8.E_align_x_AT1_AT2.py:56-117) is

    set_seed(it % 30000); z = randn(B, 512)
    w1 = Gm(z, coefs); imgs1 = Gs.forward(w1, lod)                     (no grad)
    const2, w2 = E(imgs1); imgs2 = Gs.forward(w2, lod)
    loss_imgs, 5*loss_medium, 9*loss_small      ONE evaluation, three gradient images (losses.image_losses_split)
    for each of them, in this order:  zero_grad; backward(retain_graph); LREQAdam.step
    loss_mslv = (space_loss(w1, w2) + space_loss(const1, const2)) * 0.01 -> zero_grad; backward; step

All three window gradients w.r.t. imgs2 are formed before the first optimizer step, as in the reference (imgs2 is computed once);
what changes from phase to phase is the encoder: every backward reads the weights the previous step left (the
version-keyed weight cache re-packs them) - except the data gradient of E_Blur's strided conv_2, which in the reference convolves
with a tensor derived from the weight at forward time (transform_kernel, model/utils/lreq.py:145-147) that autograd saves: it
keeps the forward's values through all four backward passes, and so it does here.  The scripts lower on the ladder leave phases out (`image_phases`, `latent_terms`,
PRESETS).  zero_grad() drops the gradients (torch >= 2.0): a parameter without a gradient in a phase is skipped by LREQAdam.

Eager launches only: capture() raises (a replayed graph of the four-phase iteration has not been validated).  Single process,
--mtype 1 and 2, E_Blur only; everything else raises.
"""
import os

import torch
import torch.distributed as dist

from . import losses, models, ops
from .generators import generator_family
from .train_step import TrainStep

IMAGE_PHASES = ("imgs", "AT1", "AT2")          # the order of the scripts' optimizer steps; also the window order of the loss
LATENT_TERMS = ("w", "c")

# --preset: (image phases, latent terms, latent scale) of each script's loop body
PRESETS = {
    "ablation4": (("imgs",), ("w",), 0.01),                        # 4.E_align_w_zn.py:72-90 (loss_c commented out)
    "ablation5": (("imgs",), ("w", "c"), 0.01),                    # 5.E_align_w_zn_zc.py:73-91
    "ablation6": (("imgs",), ("w", "c"), 0.01),                    # 6.E_align_x.py:73-91
    "ablation7": (("imgs", "AT1"), ("w", "c"), 0.01),              # 7.E_align_x_AT1.py:73-99
    "ablation8": (("imgs", "AT1", "AT2"), ("w", "c"), 0.01),       # 8.E_align_x_AT1_AT2.py:73-117
    "cat256": (("imgs", "AT1", "AT2"), ("w",), 1.0),               # Cat256/E_align_case_2.py:185-228 (loss_w alone, unscaled)
}


def _names(what, given, known):
    given = tuple(given)
    if not given:
        raise ValueError(f"Case2Step: {what} is empty; choose from {known}")
    for n in given:
        if n not in known:
            raise ValueError(f"Case2Step: unknown name {n!r} in {what}; supported: {known}")
    if len(set(given)) != len(given):
        raise ValueError(f"Case2Step: {what} = {given} names an entry twice; each of {known} at most once")
    return tuple(n for n in known if n in given)          # the scripts' order


class Case2Step(TrainStep):
    def __init__(self, generator, E, lpips_model, mapping=None, image_phases=IMAGE_PHASES, latent_terms=LATENT_TERMS,
                 latent_scale=0.01, lr=0.0015, beta_1=0.0, batch_size=2, z_dim=512, reference_noise=False):
        """`generator` + `mapping`: the StyleGAN1 Gs and Gm (mtype 1), or a StyleGAN2Generator alone (mtype 2; latent term `w`
        only).  `E`: encoder_variants.BlurBE, or its noise-free forms BlurBEW / BlurBEW2 (dge_amd.e_align_w).  `image_phases`: which of imgs / AT1 / AT2 get an optimizer step of their own;
        `latent_terms`: the terms of the last step's loss, (sum of terms) * latent_scale."""
        from .encoder_variants import BlurBE, BlurBEW
        self.image_phases = _names("image_phases", image_phases, IMAGE_PHASES)
        self.latent_terms = _names("latent_terms", latent_terms, LATENT_TERMS)
        family = generator_family(generator)
        if family in ("pggan", "biggan"):
            raise ValueError("Case2Step: --mtype 3 (PGGAN) and 4 (BigGAN) have no case-2 script with E_Blur; supported: StyleGAN1 "
                             "(Gs with mapping=Gm) and StyleGAN2")
        if mapping is None and family != "stylegan2":
            raise ValueError("Case2Step: pass the StyleGAN1 synthesis network together with mapping=Gm (mtype 1) or a "
                             "StyleGAN2Generator (mtype 2)")
        if not isinstance(E, (BlurBE, BlurBEW)):            # (BlurBEW2 is a BlurBEW)
            raise ValueError(f"Case2Step: case 2 trains the E_Blur encoder (encoder_variants.BlurBE, BlurBEW, BlurBEW2), got "
                             f"{type(E).__name__}; E.BE belongs to case 1 (e_align.EAlignStep)")
        if mapping is None and "c" in self.latent_terms:
            raise ValueError("Case2Step: latent term 'c' is not offered for StyleGAN2: Cat256/E_align_case_2.py:221-228 logs loss_c "
                             "and trains on loss_w alone; use latent_terms=('w',)")
        if dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or os.environ.get("DGE_FORCE_DIST") == "1"):
            raise RuntimeError("Case2Step runs in a single process (the case-2 scripts have no data-parallel form)")
        super().__init__(generator, E, lpips_model, mapping=mapping, lr=lr, beta_1=beta_1, batch_size=batch_size, z_dim=z_dim,
                         reference_noise=reference_noise)
        self.latent_scale = float(latent_scale)
        # phases 2.. back-propagate after optimizer steps: the strided conv_2 of E_Blur then reads the forward's weights in the
        # reference, every other layer the live ones (autograd_encblur.blur_encoder_forward)
        E.__dict__["_conv2_dgrad_at_forward"] = True
        self.const1 = None

    def capture(self, *a, **k):
        raise RuntimeError("Case2Step: hipGraph capture is not offered (eager launches only)")

    def _encoder_noises(self, R):
        """reference_noise: the reference's own sequence of CPU draws (model/E/E_Blur.py: two per block, the second at half
        resolution where conv_2 is strided; one for the last block)."""
        if not getattr(self.E, "noise", True):         # E_Blur_W / E_Blur_W_2 draw none: nothing to replay
            return None
        out = []
        B = self.batch_size
        for j, blk in enumerate(self.E.decode_block):
            r = R >> j
            out.append(torch.randn(B, 1, r, r))
            if blk.has_last_conv:
                r2 = r // 2 if blk.fused_scale else r
                out.append(torch.randn(B, 1, r2, r2))
        return [n.to(self.dev) for n in out]

    def step(self, iteration, z=None, noises=None, gen_noises=(None, None), new_z=None, prefetch_next=False):
        """One iteration; `z`, `noises` (encoder), `gen_noises` (StyleGAN1: first / second pass) and `new_z` (StyleGAN2 style
        mixing) replay captured reference inputs in parity runs.  Returns `self.last` (detached tensors, no host synchronisation)."""
        if prefetch_next:
            raise ValueError("Case2Step.step: prefetch_next is not offered (the generator pass opens its own iteration)")
        z, imgs1, w1, const2, w2, imgs2 = self._head(iteration, z, noises, gen_noises, new_z)

        # every window's loss and gradient image from one evaluation, in front of the first optimizer step
        on = tuple(n in self.image_phases for n in IMAGE_PHASES)
        img_losses, info_img = losses.image_losses_split(imgs1, imgs2, self.lpips, windows=on)
        for k, name in enumerate(IMAGE_PHASES):
            if on[k]:
                self.opt.zero_grad()
                img_losses[k].backward(retain_graph=True)
                self.opt.step()

        loss_w = loss_c = info_w = info_c = None
        total = None
        if "w" in self.latent_terms:
            loss_w, info_w = losses.space_loss(w1, w2, image_space=False)
            total = loss_w
        if "c" in self.latent_terms:
            if self.const1 is None or self.const1.shape[0] != self.batch_size:
                self.const1 = self.G.const.detach().repeat(self.batch_size, 1, 1, 1).float().clone()         # 8.E_align_x_AT1_AT2.py:30-31
            loss_c, info_c = losses.space_loss(self.const1, const2, image_space=False)
            total = loss_c if total is None else total + loss_c
        loss_mslv = total * self.latent_scale if self.latent_scale != 1.0 else total
        self.opt.zero_grad()
        loss_mslv.backward()
        self.opt.step()
        ops.zero_arena_end()
        det = self.det
        self.last = dict(imgs1=imgs1, imgs2=det(imgs2), w1=det(w1), w2=det(w2), const2=det(const2), info_img=info_img,
                         phase_losses={n: det(img_losses[k]) for k, n in enumerate(IMAGE_PHASES) if on[k]},
                         loss_imgs=det(img_losses[0]), loss_medium=det(img_losses[1]), loss_small=det(img_losses[2]),
                         loss_mslv=det(loss_mslv), loss_w=det(loss_w), loss_c=det(loss_c), info_w=info_w, info_c=info_c)
        return self.last


def build_models(mtype=1, img_size=256, start_features=64, compute_dtype="bf16", device="cuda", lpips=True, seed=0):
    """(G, Gm | None, E_Blur, LPIPS | None) with seeded random-init weights (tests, the timing tool); no checkpoints ship."""
    if mtype == 1:
        Gs, Gm, _, LP = models.build_models_sg1(img_size, start_features, compute_dtype, device=device, lpips=lpips, seed=seed, encoder=False)
    elif mtype == 2:
        Gs, _, LP = models.build_models(img_size, start_features, compute_dtype, device=device, lpips=lpips, seed=seed)
        Gm = None
    else:
        raise ValueError("case 2 is offered for --mtype 1 (StyleGAN1) and 2 (StyleGAN2)")
    return Gs, Gm, models.blur_encoder(img_size, start_features, compute_dtype, device), LP


def load_models(args, device="cuda", lpips=True):
    """Generator checkpoints through models.load_models; the encoder is E_Blur with the optional --checkpoint_dir_E state_dict."""
    if args.mtype not in (1, 2):
        raise ValueError("case 2 is offered for --mtype 1 (StyleGAN1) and 2 (StyleGAN2); 3 and 4 have no E_Blur case-2 script")
    G, Gm, _, LP = models.load_models(args, device=device, lpips=lpips, encoder=False)
    E = models.blur_encoder(args.img_size, args.start_features, getattr(args, "compute_dtype", "bf16"), device)
    if args.checkpoint_dir_E is not None:
        E.load_state_dict(torch.load(args.checkpoint_dir_E, map_location="cpu"))
    return G, Gm, E, LP


def resolve_recipe(args):
    """(image phases, latent terms, latent scale): --preset first, then whatever of --phases / --latent / --latent_scale is given."""
    phases, latent, scale = PRESETS[args.preset] if args.preset else (IMAGE_PHASES, LATENT_TERMS if args.mtype == 1 else ("w",),
                                                                     0.01 if args.mtype == 1 else 1.0)
    if args.phases is not None:
        phases = tuple(s for s in args.phases.split(",") if s)
    if args.latent is not None:
        latent = tuple(s for s in args.latent.split(",") if s)
    if args.latent_scale is not None:
        scale = args.latent_scale
    return tuple(phases), tuple(latent), float(scale)


def train(tensor_writer=None, args=None):
    """The scripts' train(): info rows printed every iteration there, written to Loss.txt every 100 (here: printed every 100),
    E_model_ep%d_iter%d.pth every 5000 (8.E_align_x_AT1_AT2.py:175-190)."""
    phases, latent, scale = resolve_recipe(args)
    G, Gm, E, LP = load_models(args)
    models.prepare_training(args, LP)
    st = Case2Step(G, E, LP, mapping=Gm, image_phases=phases, latent_terms=latent, latent_scale=scale, lr=args.lr,
                   beta_1=args.beta_1, batch_size=args.batch_size, z_dim=args.z_dim)
    out_dir = args.experiment_dir
    if out_dir:
        os.makedirs(os.path.join(out_dir, "models"), exist_ok=True)
    for iteration in range(args.iterations):
        r = st.step(iteration)
        if iteration % 100 == 0:
            tag = "ep_%d_iter_%d" % (iteration // 30000, iteration % 30000)
            info = r["info_img"].cpu().tolist()
            print(tag, *["loss_%s %.6f" % (n, float(v)) for n, v in r["phase_losses"].items()], "loss_mslv %.6f" % float(r["loss_mslv"]))
            for k, n in enumerate(IMAGE_PHASES):
                if n in st.image_phases:          # a script prints the rows of the crops it computes
                    print("loss_%s_info: %s" % (n, info[k][1:]))
            for n in st.latent_terms:
                print("loss_%s_info: %s" % (n, r["info_" + n].cpu().tolist()[1:]))
            if out_dir:
                with open(os.path.join(out_dir, "Loss.txt"), "a+") as f:
                    print("i_" + str(iteration), {n: float(v) for n, v in r["phase_losses"].items()}, float(r["loss_mslv"]), file=f)
                if iteration % 5000 == 0:
                    torch.save(E.state_dict(), os.path.join(out_dir, "models", "E_model_ep%d_iter%d.pth" % (iteration // 30000, iteration % 30000)))
    return st


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="the training args (case 2: one optimizer step per loss, E_Blur)")
    models.add_train_args(parser, iterations=60001)
    models.add_model_args(parser)
    parser.set_defaults(mtype=1)
    # not in the reference
    parser.add_argument("--preset", choices=sorted(PRESETS), default=None, help="the loop body of one script: sets --phases, --latent, --latent_scale")
    parser.add_argument("--phases", default=None, help="image losses with an optimizer step of their own, e.g. imgs,AT1,AT2")
    parser.add_argument("--latent", default=None, help="terms of the latent loss: w or w,c")
    parser.add_argument("--latent_scale", type=float, default=None)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.mtype not in (1, 2):
        print("error")            # the scripts print it for a model type they do not handle
        raise SystemExit(2)
    return train(None, args)


if __name__ == "__main__":
    main()
