"""Model construction, checkpoint loading and the command-line flags that the training and inference entry points share."""
import math

import torch

from .biggan_generator import BigGAN, BigGANConfig
from .encoder import BE
from .encoder_variants import BigBE, BlurBE, BlurBEW, BlurBEW2, BlurBEZ, PGBE
from .lpips import LPIPS
from .pggan_generator import PGGANGenerator
from .stylegan1 import Generator, Mapping
from .stylegan2_generator import StyleGAN2Generator


def imgs_px(G):
    """pixels of one generated image (resolution attribute of the generator families; 0 when unknown)"""
    r = getattr(G, "resolution", None) or getattr(G, "img_size", None) or 0
    return int(r) * int(r)


def _freeze(G, noise=None):
    """G's weight gradients are never used; the noise strengths (parameters named `noise`) of a seeded init are 0.05"""
    with torch.no_grad():
        for name, p in G.named_parameters():
            p.requires_grad_(False)
            if noise and noise in name:
                p.fill_(0.05)


def build_models(img_size=1024, start_features=16, compute_dtype="bf16", device="cuda", lpips=True, seed=0,
                 fmaps_base=32 << 10, fmaps_max=512, enc_maxf=512, encoder=True):
    """Models of BASELINE config 3 with seeded random-init weights (no checkpoints ship; encoder=False: E is None)."""
    torch.manual_seed(seed)
    G = StyleGAN2Generator(img_size, fmaps_base=fmaps_base, fmaps_max=fmaps_max, compute_dtype=compute_dtype).to(device)
    _freeze(G, noise="noise_strength")
    E = BE(startf=start_features, maxf=enc_maxf, layer_count=int(math.log2(img_size) - 1), compute_dtype=compute_dtype).to(device) if encoder else None
    return G, E, (LPIPS(compute_dtype=compute_dtype).to(device) if lpips else None)


def build_models_sg1(img_size=256, start_features=64, compute_dtype="bf16", device="cuda", lpips=True, seed=0, encoder=True):
    """Models of BASELINE config 2 (StyleGAN1, E_align_s2.py:27-46) with seeded random-init weights (encoder=False: E is None)."""
    torch.manual_seed(seed)
    L = int(math.log2(img_size) - 1)
    Gs = Generator(startf=start_features, maxf=512, layer_count=L, latent_size=512, channels=3, compute_dtype=compute_dtype).to(device)
    Gm = Mapping(num_layers=2 * L, mapping_layers=8, latent_size=512, dlatent_size=512, mapping_fmaps=512).to(device)
    _freeze(Gs, noise="noise_weight")
    _freeze(Gm)
    Gm.buffer1 = torch.randn(2 * L, 512) * 0.1
    E = BE(startf=start_features, maxf=512, layer_count=L, compute_dtype=compute_dtype).to(device) if encoder else None
    return Gs, Gm, E, (LPIPS(compute_dtype=compute_dtype).to(device) if lpips else None)


def build_models_pg(img_size=256, start_features=64, compute_dtype="bf16", device="cuda", lpips=True, seed=0, encoder=True):
    """Models of BASELINE config 1 (PGGAN, E_align_s2.py:67-77) with seeded random-init weights."""
    torch.manual_seed(seed)
    G = PGGANGenerator(resolution=img_size, compute_dtype=compute_dtype).to(device)
    _freeze(G)
    E = PGBE(startf=start_features, maxf=512, layer_count=int(math.log2(img_size) - 1), pggan=True, compute_dtype=compute_dtype).to(device) if encoder else None
    return G, E, (LPIPS(compute_dtype=compute_dtype).to(device) if lpips else None)


def build_models_big(config, img_size=256, start_features=64, compute_dtype="bf16", device="cuda", lpips=True, seed=0, encoder=True):
    """Models of BASELINE config 4 (BigGAN-deep, E_align_s2.py:79-86) with seeded random-init weights; `config`: BigGANConfig."""
    torch.manual_seed(seed)
    G = BigGAN(config, compute_dtype=compute_dtype).to(device)
    _freeze(G)
    E = BigBE(startf=start_features, maxf=512, layer_count=int(math.log2(img_size) - 1), biggan=True, compute_dtype=compute_dtype).to(device) if encoder else None
    return G, E, (LPIPS(compute_dtype=compute_dtype).to(device) if lpips else None)


BLUR_VARIANTS = {None: BlurBE, "z": BlurBEZ, "w": BlurBEW, "w_2": BlurBEW2}


def blur_encoder(img_size, start_features, compute_dtype, device, z_space=False, maxf=512, variant=None):
    """E_Blur (encoder_variants.BlurBE), or with z_space its Z-code form E_Blur_Z (BlurBEZ), sized for `img_size`.
    `variant`: "w" / "w_2" for the noise-free W-space forms E_Blur_W / E_Blur_W_2 (BlurBEW, BlurBEW2), "z" = z_space."""
    if variant not in BLUR_VARIANTS:
        raise ValueError(f"blur_encoder: unknown variant {variant!r}; supported: {sorted(k for k in BLUR_VARIANTS if k)}")
    if z_space and variant not in (None, "z"):
        raise ValueError("blur_encoder: z_space goes with variant 'z' only")
    cls = BlurBEZ if z_space else BLUR_VARIANTS[variant]
    return cls(startf=start_features, maxf=maxf, layer_count=int(math.log2(img_size) - 1), latent_size=512,
               compute_dtype=compute_dtype).to(device)


def load_lpips_weights(LP, vgg_weights=None, lin_weights=None, allow_standin=False):
    """The `2*lpips` term of every image loss (training_utils.py:93) is only the reference's objective with the real
    LPIPS-VGG16 weights.  With the two files (see LPIPS.load_pretrained / INTEGRATION.md) they are loaded; without them
    training is refused unless `allow_standin` (benchmarks, smoke runs), and then says so loudly."""
    if LP is None:
        return None
    if vgg_weights:
        LP.load_pretrained(vgg_weights, lin_weights)
        return LP
    msg = ("LPIPS runs on SEEDED STAND-IN weights (no --vgg_weights / --lpips_weights given): the 2*lpips term of the image "
           "losses is a random-feature distance, NOT the reference's objective")
    if not allow_standin:
        raise RuntimeError(msg + "; pass --vgg_weights vgg16-397923af.pth --lpips_weights <lpips>/weights/v0.1/vgg.pth, "
                           "or --allow_standin_lpips for throughput / plumbing runs")
    import sys
    import warnings
    warnings.warn(msg)
    print("WARNING: " + msg, file=sys.stderr)
    return LP


def load_models(args, device="cuda", lpips=True, encoder=True):
    """Models + checkpoints of one --mtype, shared by the training and the inference entry points.  The three
    checkpoint containers of the reference: mtype 2 / 3 a dict holding `generator_smooth` (or `generator`)
    (E_align_s2.py:51-55, :67-77); mtype 1 a DIRECTORY with Gs_dict.pth, Gm_dict.pth and center_tensor.pt (:30-35);
    mtype 4 a bare state_dict next to --config_dir (:79-86); the encoder is a bare state_dict (--checkpoint_dir_E).
    Everything is read with map_location='cpu' and moved by load_state_dict.  Returns (G, Gm | None, E, LP | None).
    encoder=False (callers with an encoder of their own): no E is built and --checkpoint_dir_E is not read, E is None."""
    cd = getattr(args, "compute_dtype", "bf16")
    small = {k: getattr(args, k) for k in ("fmaps_base", "fmaps_max", "enc_maxf") if getattr(args, k, None) is not None}
    Gm = None
    if args.mtype in (2, 3):
        build, widths = (build_models, small) if args.mtype == 2 else (build_models_pg, {})
        G, E, LP = build(args.img_size, args.start_features, cd, device=device, lpips=lpips, encoder=encoder, **widths)
        if args.checkpoint_dir_GAN:
            ckpt = torch.load(args.checkpoint_dir_GAN, map_location="cpu")
            G.load_state_dict(ckpt["generator_smooth"] if "generator_smooth" in ckpt else ckpt["generator"])
    elif args.mtype == 1:
        G, Gm, E, LP = build_models_sg1(args.img_size, args.start_features, cd, device=device, lpips=lpips, encoder=encoder)
        if args.checkpoint_dir_GAN:                 # E_align_s2.py:30-35: a directory holding the three files
            G.load_state_dict(torch.load(args.checkpoint_dir_GAN + "Gs_dict.pth", map_location="cpu"))
            Gm.load_state_dict(torch.load(args.checkpoint_dir_GAN + "Gm_dict.pth", map_location="cpu"))
            Gm.buffer1 = torch.load(args.checkpoint_dir_GAN + "./center_tensor.pt", map_location="cpu")
    elif args.mtype == 4:
        G, E, LP = build_models_big(BigGANConfig.from_json_file(args.config_dir), args.img_size, args.start_features, cd,
                                    device=device, lpips=lpips, encoder=encoder)
        if args.checkpoint_dir_GAN:
            G.load_state_dict(torch.load(args.checkpoint_dir_GAN, map_location="cpu"))
    else:
        raise ValueError("--mtype must be 1 (StyleGAN1), 2 (StyleGAN2), 3 (PGGAN) or 4 (BigGAN)")
    if E is not None and getattr(args, "checkpoint_dir_E", None) is not None:
        E.load_state_dict(torch.load(args.checkpoint_dir_E, map_location="cpu"))
    return G, Gm, E, LP


def add_model_args(parser):
    """The reference's model flags (E_align_s2.py:304-318), shared by the training and inference parsers."""
    parser.add_argument("--checkpoint_dir_GAN", default=None)
    parser.add_argument("--config_dir", default=None)
    parser.add_argument("--checkpoint_dir_E", default=None)
    parser.add_argument("--img_size", type=int, default=1024)
    parser.add_argument("--img_channels", type=int, default=3)
    parser.add_argument("--z_dim", type=int, default=512)
    parser.add_argument("--mtype", type=int, default=2)
    parser.add_argument("--start_features", type=int, default=16)
    parser.add_argument("--compute_dtype", default="bf16")
    # not in the reference: reduced StyleGAN2 / encoder widths (tests, smoke runs)
    parser.add_argument("--fmaps_base", type=int, default=None)
    parser.add_argument("--fmaps_max", type=int, default=None)
    parser.add_argument("--enc_maxf", type=int, default=None)
    return parser


def add_train_args(parser, iterations=210000):
    """The reference's loop flags (E_align_s2.py:304-308) and, not in the reference, the LPIPS weights and the deterministic switch."""
    parser.add_argument("--iterations", type=int, default=iterations)
    parser.add_argument("--lr", type=float, default=0.0015)
    parser.add_argument("--beta_1", type=float, default=0.0)
    parser.add_argument("--batch_size", type=int, default=2)
    parser.add_argument("--experiment_dir", default=None)
    parser.add_argument("--vgg_weights", default=None, help="torchvision vgg16 checkpoint (features.*) or an lpips.LPIPS state_dict")
    parser.add_argument("--lpips_weights", default=None, help="the lpips package's weights/v0.1/vgg.pth (lin{k}.model.1.weight)")
    parser.add_argument("--deterministic", action="store_true", help="bit-reproducible reductions (training_utils.py:51 cudnn.deterministic): ops.set_deterministic")
    parser.add_argument("--allow_standin_lpips", action="store_true", help="train on seeded stand-in LPIPS weights (NOT the reference objective)")
    return parser


def prepare_training(args, LP):
    """The head of every train(): the deterministic switch and the LPIPS weight guard."""
    if getattr(args, "deterministic", False):
        from . import ops
        ops.set_deterministic(True)
    return load_lpips_weights(LP, getattr(args, "vgg_weights", None), getattr(args, "lpips_weights", None),
                              allow_standin=getattr(args, "allow_standin_lpips", False))
