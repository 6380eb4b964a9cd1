"""Real-image inversion with a PGGAN generator and the E_PG encoder `--mtype 3` trains, on the HIP path.

The reference has no PGGAN inversion script.  This is the v2 loop of embedding_v2_styleGAN1.py:71-189
(embedding_v2.LatentEmbedStep, generator kind "pg") applied to PGGAN + E_PG in the evident-intent form of SURVEY Q5: the
encoder's latent is the live output of its `new_final` head, as in `e_align --mtype 3`.

  mode "E" (--optimizeE true):  the encoder is re-loaded per image group and fine-tuned; z = E(imgs1) every iteration.
  mode "W" (--optimizeE false): the encoder is frozen and the latent z [B,512] itself is optimised (LREQAdam on the leaf z); the
                                encoder backward of phase 2 runs in its data-only form (pg_encoder_backward(params=False)).

Per iteration:

    [E] _, z = E(imgs1);   imgs2 = G(z, fused_backward=True)["image"];   _, w2 = E(imgs2)      (StyleGAN1's order: before the step)
    loss_msiv = L(img) + 0.375*L(medium) + 0.625*L(small)       (embedding_v2.IMG_WEIGHTS; all three windows carry gradient)
    zero_grad; loss_msiv.backward(retain_graph=True); step
    loss_msLv = 0.01*space_loss(z, w2) + beta*||z||_p;  zero_grad; backward; step

Phase 2 back-propagates space_loss(z, w2) through E_PG into the generated image (the encoder's image gradient) and on through the
generator's fused backward (ops.pixelnorm_act_bwd between its data-gradient convs).

Decisions (none of them is taken from a PGGAN script: there is none):
  * There is no const term: E_PG returns (0, z), so the space_loss(const2, const3) term of the StyleGAN loops has no operand.
  * The mode-W start code is E(imgs1) detached, or `w_init` if given (StyleGAN1's start; a random z would start far from the image).
  * The defaults are StyleGAN1's: iterations 1501, lr 0.005, beta_1 0, beta 1e-3, norm_p 2, and the tracker rules are
    tracker_rules("sg1", iterations) - armed at iterations // 2, hysteresis 1.05, minima restart per group.
  * capture() / replay() are those of every LatentEmbedStep (embed_step.TwoPhaseEmbedStep): E_PG's noise draws go through enc_steps.draw_noises and the device seed scalar, the
    generator is called with lod=0 (validated once here: the captured iteration cannot read the `lod` buffer back).
  * independent=True (mode W): one tracker per row, per-row losses, ||z[b]||_p per row, as embedding_v2 describes it.
  * Refused with a message: independent with mode E, more than one process, --encoder be, --truncation (PGGAN has neither a W+
    code to truncate nor an E.BE head for z).
  * Checkpoints come in the containers models.load_models reads for --mtype 3: the generator a dict holding `generator_smooth`
    (or `generator`), the encoder a bare state_dict.
"""
import argparse
import math

import torch

from . import ops
from .embed_step import several_processes
from .embedding_v2 import DEFAULTS as _V2_DEFAULTS, LatentEmbedStep, _refuse, add_inversion_args, invert_group, load_generator_smooth, \
    open_run, run_inversion

DEFAULTS = {k: _V2_DEFAULTS[1][k] for k in ("iterations", "lr", "beta_1", "beta", "norm_p")}          # StyleGAN1's
MSG_INDEPENDENT = "PGEmbedStep: independent=True needs mode 'W': in mode 'E' one encoder is shared by the rows of a group"
MSG_DIST = "PGEmbedStep: more than one process is not offered (the inversion loop is a single-process loop)"
MSG_ENCODER = "embedding_v2_pggan: --encoder is not offered (E_PG is the encoder with a z head; E.BE and E_Blur encode into W+)"
MSG_TRUNCATION = "embedding_v2_pggan: --truncation is not offered (PGGAN has no W+ code and no average latent to truncate towards)"


class PGEmbedStep(LatentEmbedStep):
    """LatentEmbedStep on z [B, z_space_dim] with a PGGANGenerator and an E_PG encoder (encoder_variants.PGBE, pggan=True)."""

    def __init__(self, G, E, lpips_model, mode="E", lr=None, beta_1=None, beta=None, norm_p=None, iterations=None, arm_iter=None,
                 events_cap=256, seed=0, independent=False):
        if independent and mode == "E":
            raise ValueError(MSG_INDEPENDENT)
        if several_processes():
            raise ValueError(MSG_DIST)
        if not getattr(E, "pggan", False):
            raise ValueError("PGEmbedStep: the encoder needs its z head (PGBE(pggan=True))")
        if float(G.lod) != 0:
            raise ValueError("PGEmbedStep: only a fully grown generator (lod == 0) is implemented")
        d = DEFAULTS
        super().__init__(G, E, lpips_model, mode=mode, generator="pg", lr=d["lr"] if lr is None else lr,
                         beta_1=d["beta_1"] if beta_1 is None else beta_1, beta=beta, norm_p=d["norm_p"] if norm_p is None else norm_p,
                         iterations=iterations, arm_iter=arm_iter, events_cap=events_cap, seed=seed, independent=independent)
        for p in G.parameters():
            p.requires_grad_(False)


def _loss_txt_infos(r):
    """The result dict with the info vectors under the names embedding_v2.dump_group prints (window rows of info_img)."""
    img = r["info_img"]
    return dict(r, info_imgs=img.select(-2, 0), info_Gcam=img.select(-2, 1), info_mask=img.select(-2, 2))


def invert_pg(st, imgs1, iterations, launch="graph", save_every=100, out_dir=None, group=0, w_init=None, keep=None):
    """`iterations` iterations on one image group, as embedding_v2.invert_v2 (launch="graph": the iteration is captured once and
    replayed; later groups go through set_image).  With `out_dir` the every-`save_every` dumps (image pair, per-row z, a Loss.txt
    block) and, at the end, the tracker's files.  Returns the last result dict with the tracker read-out under "tracker"."""
    return invert_group(st, imgs1, iterations, launch, save_every, out_dir, group, keep, dict(w_init=w_init), dict(loss_txt=True),
                        infos=_loss_txt_infos)


def build_models_pg_v2(img_size=1024, start_features=16, compute_dtype="bf16", device="cuda", seed=0, lpips=True, fmaps_base=None,
                       fmaps_max=None, enc_maxf=None):
    """PGGANGenerator(img_size) (frozen) + PGBE(start_features, enc_maxf or 512, log2(img_size) - 1, pggan=True) + LPIPS, seeded
    random-init weights: models.build_models_pg with the reduced widths of tests and smoke runs."""
    from .encoder_variants import PGBE
    from .lpips import LPIPS
    from .pggan_generator import PGGANGenerator
    torch.manual_seed(seed)
    kw = {k: v for k, v in (("fmaps_base", fmaps_base), ("fmaps_max", fmaps_max)) if v is not None}
    G = PGGANGenerator(resolution=img_size, compute_dtype=compute_dtype, **kw).to(device)
    for p in G.parameters():
        p.requires_grad_(False)
    E = PGBE(startf=start_features, maxf=enc_maxf or 512, layer_count=int(math.log2(img_size) - 1), pggan=True,
             compute_dtype=compute_dtype).to(device)
    return G, E, (LPIPS(compute_dtype=compute_dtype).to(device) if lpips else None)


def load_checkpoints(G, E, gan=None, enc=None):
    """The --mtype 3 containers of models.load_models: the generator a dict holding `generator_smooth` (or `generator`), the encoder
    a bare state_dict."""
    if gan:
        load_generator_smooth(G, gan)
    if enc:
        E.load_state_dict(torch.load(enc, map_location="cpu"))


# ------------------------------------------------------------------ CLI
def make_parser():
    p = argparse.ArgumentParser(description="PGGAN real-image inversion with the E_PG encoder (the v2 loop of embedding_v2_styleGAN1.py)")
    add_inversion_args(p, DEFAULTS, 3, "./real_imgs/", "z")
    p.add_argument("--beta", type=float, default=DEFAULTS["beta"], help="weight of ||z||_p")
    p.add_argument("--norm_p", type=int, default=DEFAULTS["norm_p"], help="p of ||z||_p")
    p.add_argument("--encoder", type=_refuse(MSG_ENCODER), default=None, help="not offered: E_PG is the encoder of this loop")
    p.add_argument("--truncation", type=_refuse(MSG_TRUNCATION), default=None, help="not offered: PGGAN has no W+ code")
    return p


def parse_args(argv=None):
    args = make_parser().parse_args(argv)
    if args.mtype != 3:
        raise SystemExit("embedding_v2_pggan: --mtype is 3 (PGGAN + E_PG); the StyleGAN loops are dge_amd.embedding_v2, BigGAN's is "
                         "dge_amd.embedding_v2_biggan")
    if args.independent and args.optimizeE:
        raise SystemExit("embedding_v2_pggan: --independent true needs --optimizeE false (the fine-tuned encoder is shared by a group)")
    if several_processes(env=True):
        raise SystemExit("embedding_v2_pggan: " + MSG_DIST.split(": ", 1)[1])
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.deterministic:
        ops.set_deterministic(True)
    dev = "cuda"
    G, E, LP = build_models_pg_v2(args.img_size, args.start_features, args.compute_dtype, device=dev, seed=args.seed,
                                  fmaps_base=args.fmaps_base, fmaps_max=args.fmaps_max, enc_maxf=args.enc_maxf)
    load_checkpoints(G, E, args.checkpoint_dir_GAN, args.checkpoint_dir_E)
    out, imgs = open_run(args, LP, "./realimg_embedding_result/pggan", dev)
    st = PGEmbedStep(G, E, LP, mode="E" if args.optimizeE else "W", lr=args.lr, beta_1=args.beta_1, beta=args.beta, norm_p=args.norm_p,
                     iterations=args.iterations, seed=args.seed, independent=args.independent)
    return run_inversion(args, st, invert_pg, imgs, out)


if __name__ == "__main__":
    main()
