"""Z-space encoder training: the first ablation of the reference (ablation_utils/1.E_align_z.py:17-149) on the HIP path.

The encoder E_Blur_Z (encoder_variants.BlurBEZ) predicts the Z code; the image loss back-propagates through the StyleGAN1
synthesis network AND the mapping network into it.  One iteration (`EAlignZStep.step`, :58-92):

    set_seed(it % 30000); z_c1 = randn(B, 512)
    w1 = Gm(z_c1, coefs); imgs1 = Gs.forward(w1, lod)                 (no grad: nothing in it reaches E)
    z_c2 = E(imgs1)[0].squeeze(-1).squeeze(-1)
    w2 = Gm(z_c2, coefs); imgs2 = Gs.forward(w2, lod)                 (grad: Mapping's dge_mapping_bwd, Gs's DecodeFunction)
    loss_imgs = space_loss(imgs1, imgs2, lpips)   -> zero_grad, backward(retain_graph), step     (full image only, no crops)
    loss_c    = space_loss(z_c1, z_c2, image_space=False) * 0.01 -> zero_grad, backward, step

The second backward runs on the weights the first step already updated, as in the reference.  No weight gradient
of Gs or Gm is formed (the reference accumulates them, no optimizer reads them).  StyleGAN1 only (--mtype 1, the
reference prints `error` for any other type); single process only.
"""
import os

import torch
import torch.distributed as dist

from . import losses, models
from .train_step import TrainStep


class EAlignZStep(TrainStep):
    def __init__(self, Gs, Gm, E, lpips_model, lr=0.0015, beta_1=0.0, batch_size=2, z_dim=512):
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise RuntimeError("EAlignZStep runs in a single process (1.E_align_z.py has no data-parallel form)")
        super().__init__(Gs, E, lpips_model, mapping=Gm, lr=lr, beta_1=beta_1, batch_size=batch_size, z_dim=z_dim)
        self.Gm = Gm

    def step(self, iteration, z=None, gen_noises=(None, None)):
        """`z`: optional z_c1 [B, 512] (parity runs), else drawn after set_seed(iteration % 30000) on the CPU generator as the
        reference does; `gen_noises`: optional (first, second) lists of StyleGAN1 noise tensors in the reference's draw order."""
        if z is None:
            z = self._draw_z(iteration)
        z_c1 = z.to(self.dev, non_blocking=True).float().contiguous()
        with torch.no_grad():
            imgs1, w1 = self.gen.sample(z_c1, gen_noises[0])
        z_c2, _ = self.E(imgs1)
        z_c2 = z_c2.squeeze(-1).squeeze(-1)
        w2 = self.Gm(z_c2, coefs_m=self.gen.coefs)
        imgs2 = self.gen.synth(w2, gen_noises[1])

        loss_imgs, info_img = losses.space_loss(imgs1, imgs2, lpips_model=self.lpips)
        self.opt.zero_grad()
        loss_imgs.backward(retain_graph=True)
        self.opt.step()

        loss_c, info_c = losses.space_loss(z_c1, z_c2, image_space=False)
        loss_mslv = loss_c * 0.01
        self.opt.zero_grad()
        loss_mslv.backward()
        self.opt.step()
        det = self.det
        self.last = dict(imgs1=imgs1, imgs2=det(imgs2), w1=w1, w2=det(w2), z_c1=z_c1, z_c2=det(z_c2), loss_imgs=loss_imgs.detach(),
                         info_img=info_img, loss_c=loss_c.detach(), info_c=info_c)
        return self.last


def build_models_z(img_size=1024, start_features=16, compute_dtype="bf16", device="cuda", lpips=True):
    """Gs, Gm (seeded random init, models.build_models_sg1) and a fresh E_Blur_Z; checkpoints are loaded by `load_models`."""
    Gs, Gm, _, LP = models.build_models_sg1(img_size, start_features, compute_dtype, device=device, lpips=lpips, encoder=False)
    return Gs, Gm, models.blur_encoder(img_size, start_features, compute_dtype, device, z_space=True), LP


def load_models(args, device="cuda", lpips=True):
    """--mtype 1 only: Gs_dict.pth, Gm_dict.pth and center_tensor.pt from the --checkpoint_dir_GAN directory (1.E_align_z.py:21-29)
    through models.load_models, then E_Blur_Z with the optional --checkpoint_dir_E state_dict."""
    if args.mtype != 1:
        raise ValueError("1.E_align_z trains on StyleGAN1 only (--mtype 1); the reference prints 'error' for any other type")
    Gs, Gm, _, LP = models.load_models(args, device=device, lpips=lpips, encoder=False)
    E = models.blur_encoder(args.img_size, args.start_features, getattr(args, "compute_dtype", "bf16"), device, z_space=True)
    if args.checkpoint_dir_E is not None:
        E.load_state_dict(torch.load(args.checkpoint_dir_E, map_location="cpu"))
    return Gs, Gm, E, LP


def train(tensor_writer=None, args=None):
    """Reference 1.E_align_z.train() (flags :137-149): losses printed every 100 iterations, E_model_ep%d_iter%d.pth every 5000."""
    Gs, Gm, E, LP = load_models(args)
    models.prepare_training(args, LP)
    st = EAlignZStep(Gs, Gm, E, LP, lr=args.lr, beta_1=args.beta_1, batch_size=args.batch_size, z_dim=args.z_dim)
    out_dir = args.experiment_dir
    if out_dir:
        os.makedirs(os.path.join(out_dir, "models"), exist_ok=True)
    for iteration in range(args.iterations):
        r = st.step(iteration)
        if iteration % 100 == 0:
            print("ep_%d_iter_%d" % (iteration // 30000, iteration % 30000), "loss_imgs", float(r["loss_imgs"]),
                  "loss_c", float(r["loss_c"]))
            if iteration % 5000 == 0 and out_dir:
                torch.save(E.state_dict(), os.path.join(out_dir, "models", "E_model_ep%d_iter%d.pth" % (iteration // 30000, iteration % 30000)))
    return st


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="the training args (ablation 1: Z-space encoder)")
    models.add_train_args(parser, iterations=60001)
    models.add_model_args(parser)
    parser.set_defaults(mtype=1, checkpoint_dir_GAN="../checkpoint/stylegan_v1/ffhq1024/",
                        config_dir="./checkpoint/biggan/256/biggan-deep-256-config.json")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.mtype != 1:
        print("error")            # 1.E_align_z.py:42-44
        raise SystemExit(2)
    return train(None, args)


if __name__ == "__main__":
    main()
