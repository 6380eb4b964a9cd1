"""W-space encoder training without noise: ablations 3 and 2 of the reference (ablation_utils/3.E_align_w.py with
model/E/Ablation_Study/E_Blur_W.py, ablation_utils/2.E_align_w_2.py with E_Blur_W_2.py) on the HIP path.

    python -m dge_amd.e_align_w --variant w|w_2 --checkpoint_dir_GAN <dir>/ ...

Script 3 is script 4 (dge_amd.e_align_case2 --preset ablation4) with another encoder import; script 2 differs from 3 in the
encoder alone.  One iteration (3.E_align_w.py:56-90) is therefore Case2Step's with image_phases ("imgs",), latent_terms ("w",) and
latent scale 0.01:

    set_seed(it % 30000); z = randn(B, 512)
    w1 = Gm(z, coefs); imgs1 = Gs.forward(w1, lod)                     (no grad)
    const2, w2 = E(imgs1); imgs2 = Gs.forward(w2, lod)
    loss_imgs = space_loss(imgs1, imgs2, lpips)   -> zero_grad, backward(retain_graph), step
    loss_mslv = space_loss(w1, w2) * 0.01         -> zero_grad, backward, step

E_Blur_W is E_Blur without noise (no noise weights, no draws); E_Blur_W_2 additionally writes inver_mod2's output into both W+
rows of its block and drops inver_mod1's, so inver_mod1 never gets a gradient and LREQAdam never touches it.  The heads of both
run as one grouped launch per direction (dge_heads_rows_fwd, dge_heads_rows_bwd) instead of one dge_linear per head plus a stack
in the forward and one dge_linear_t + dge_dense_wgrad per head in each of the iteration's two backward passes.

StyleGAN1 only (--mtype 1; the scripts print `error` for any other type), eager, single process; capture() raises.
"""
import os

import torch

from . import models
from .e_align_case2 import Case2Step

VARIANTS = ("w", "w_2")          # 3.E_align_w.py (E_Blur_W), 2.E_align_w_2.py (E_Blur_W_2)


def encoder_class(variant):
    from .encoder_variants import BlurBEW, BlurBEW2
    if variant not in VARIANTS:
        raise ValueError(f"e_align_w: unknown variant {variant!r}; supported: {VARIANTS}")
    return BlurBEW if variant == "w" else BlurBEW2


class EAlignWStep(Case2Step):
    """Case2Step's iteration with the loop body of scripts 3 / 2: the image step, then the step on loss_w * 0.01."""

    def __init__(self, Gs, Gm, E, lpips_model, lr=0.0015, beta_1=0.0, batch_size=2, z_dim=512):
        from .encoder_variants import BlurBEW
        if not isinstance(E, BlurBEW):
            raise ValueError(f"EAlignWStep trains E_Blur_W or E_Blur_W_2 (encoder_variants.BlurBEW, BlurBEW2), got {type(E).__name__}")
        if Gm is None:
            raise ValueError("EAlignWStep: StyleGAN1 only - pass the synthesis network Gs and the mapping network Gm")
        super().__init__(Gs, E, lpips_model, mapping=Gm, image_phases=("imgs",), latent_terms=("w",), latent_scale=0.01, lr=lr,
                         beta_1=beta_1, batch_size=batch_size, z_dim=z_dim)

    def capture(self, *a, **k):
        raise RuntimeError("EAlignWStep: hipGraph capture is not offered (eager launches only)")


def build_models_w(variant="w", img_size=1024, start_features=16, compute_dtype="bf16", device="cuda", lpips=True):
    """Gs, Gm (seeded random init, models.build_models_sg1) and a fresh encoder of the variant; checkpoints: `load_models`."""
    encoder_class(variant)
    Gs, Gm, _, LP = models.build_models_sg1(img_size, start_features, compute_dtype, device=device, lpips=lpips, encoder=False)
    return Gs, Gm, models.blur_encoder(img_size, start_features, compute_dtype, device, variant=variant), LP


def load_models(args, device="cuda", lpips=True):
    """--mtype 1 only: Gs_dict.pth, Gm_dict.pth and center_tensor.pt from the --checkpoint_dir_GAN directory (3.E_align_w.py:20-29)
    through models.load_models, then the encoder of --variant with the optional --checkpoint_dir_E state_dict."""
    if args.mtype != 1:
        raise ValueError("2.E_align_w_2 / 3.E_align_w train on StyleGAN1 only (--mtype 1); the reference prints 'error' for any other type")
    encoder_class(args.variant)
    Gs, Gm, _, LP = models.load_models(args, device=device, lpips=lpips, encoder=False)
    E = models.blur_encoder(args.img_size, args.start_features, getattr(args, "compute_dtype", "bf16"), device, variant=args.variant)
    if args.checkpoint_dir_E is not None:
        E.load_state_dict(torch.load(args.checkpoint_dir_E, map_location="cpu"))
    return Gs, Gm, E, LP


def train(tensor_writer=None, args=None):
    """The scripts' train() (3.E_align_w.py:17-131): info rows every 100 iterations, E_model_ep%d_iter%d.pth every 5000."""
    Gs, Gm, E, LP = load_models(args)
    models.prepare_training(args, LP)
    st = EAlignWStep(Gs, Gm, E, LP, lr=args.lr, beta_1=args.beta_1, batch_size=args.batch_size, z_dim=args.z_dim)
    out_dir = args.experiment_dir
    if out_dir:
        os.makedirs(os.path.join(out_dir, "models"), exist_ok=True)
    for iteration in range(args.iterations):
        r = st.step(iteration)
        if iteration % 100 == 0:
            print("ep_%d_iter_%d" % (iteration // 30000, iteration % 30000), "loss_imgs %.6f" % float(r["loss_imgs"]),
                  "loss_mslv %.6f" % float(r["loss_mslv"]))
            print("loss_imgs_info: %s" % r["info_img"].cpu().tolist()[0][1:])
            print("loss_w_info: %s" % r["info_w"].cpu().tolist()[1:])
            if out_dir:
                with open(os.path.join(out_dir, "Loss.txt"), "a+") as f:
                    print("i_" + str(iteration), float(r["loss_imgs"]), float(r["loss_mslv"]), file=f)
                if iteration % 5000 == 0:
                    torch.save(E.state_dict(), os.path.join(out_dir, "models", "E_model_ep%d_iter%d.pth" % (iteration // 30000, iteration % 30000)))
    return st


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="the training args (ablations 3 and 2: W-space encoder without noise)")
    models.add_train_args(parser, iterations=60001)
    models.add_model_args(parser)
    parser.set_defaults(mtype=1, checkpoint_dir_GAN="../checkpoint/stylegan_v1/ffhq1024/",
                        config_dir="./checkpoint/biggan/256/biggan-deep-256-config.json")
    # not in the reference (there the script's file name chooses the encoder)
    parser.add_argument("--variant", choices=VARIANTS, default="w", help="w: 3.E_align_w.py (E_Blur_W); w_2: 2.E_align_w_2.py (E_Blur_W_2)")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.mtype != 1:
        print("error")            # 3.E_align_w.py:41-43
        raise SystemExit(2)
    return train(None, args)


if __name__ == "__main__":
    main()
