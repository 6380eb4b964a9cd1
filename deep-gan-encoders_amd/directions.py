"""Semantic directions of StyleGAN2's W space from the generator alone - no labels, no classifier, no boundary file:

* `sefa_directions` - SeFa (closed-form factorisation): the eigenvectors of A^T A, where A stacks the style affine weights
                      (`L.style.weight`, one row per style channel, scaled to unit length) of every conv and toRGB block that reads
                      one of the chosen W+ rows, in the block order of the style codes (autograd_s2.style_groups);
* `pca_directions`  - GANSpace (PCA in W): the eigenvectors of the covariance of w = mapping(z) over seeded samples, drawn and
                      mapped as `infer.style_sigma` does; sqrt(eigenvalue) is the unit of an edit (`sigma`).

Both are a 512 x 512 symmetric matrix from a tall operand (ops.gram, dge_gram) and its eigendecomposition (ops.eigh_sym,
dge_eigh_sym); a direction is a row of the result, the form `infer.edit_latent` takes, and `edit_direction` hands it there.
`save_directions` / `load_directions` keep the result as `directions.pt`.

Command line (`python -m dge_amd.directions`, the model flags of models.add_model_args):

    fit   --method sefa|pca [--rows 0-7] [--num 32] [--samples N --seed S] --out dirs.pt
    apply --directions dirs.pt --wp id0-wp.pt [--noise id0-noise.pt] --index k --amounts=-3,-1.5,0,1.5,3 [--rows 0-8] --out strip.png

`apply` writes one image row (infer.save_image_grid): the code moved by each amount (in units of sigma) along direction k in the
W+ rows of --rows.  With --noise (the projector's id{n}-noise.pt) the images are synthesis(wp, noises=...), so amount 0 reproduces
the projector's rec PNG.  Refused with a message: --mtype other than 2, more than one process, --index outside the file, rows
outside the model.  StyleGAN1, PGGAN and BigGAN are out of scope.

A lower module: it never imports the training script.
"""
import argparse
import math

import torch

from . import ops
from .autograd_s2 import style_groups
from .embed_step import several_processes

KEYS = ("directions", "eigenvalues", "sigma", "mean", "method", "rows", "samples", "seed")


def _check_rows(rows, num_layers):
    """`rows` (None: all) -> the sorted list of distinct W+ rows; ValueError for a row outside the model."""
    if rows is None:
        return list(range(num_layers))
    rows = sorted({int(r) for r in rows})
    if not rows or rows[0] < 0 or rows[-1] >= num_layers:
        raise ValueError(f"directions: rows {rows} outside the {num_layers} rows (0 .. {num_layers - 1}) of the model's W+ code")
    return rows


def _result(evals, evecs, num, sigma, mean, method, rows, samples, seed):
    K = evals.numel() if num is None else int(num)
    if not 1 <= K <= evals.numel():
        raise ValueError(f"directions: num = {num} outside 1 .. {evals.numel()}")
    return dict(directions=evecs[:K].contiguous(), eigenvalues=evals[:K].contiguous(), sigma=sigma[:K].contiguous(), mean=mean,
                method=method, rows=rows, samples=samples, seed=seed)


@torch.no_grad()
def sefa_directions(G, rows=None, num=None):
    """SeFa on the StyleGAN2 generator G: A = the style weights of every conv block and every toRGB block that reads one of the W+
    rows `rows` (default: all), in block order; M = dge_gram(A, row_norm) = sum of the outer products of A's unit rows; the
    eigenvectors of M by dge_eigh_sym, largest eigenvalue first.  Returns the dict of the module docstring with K = `num`
    directions (default: all 512); `sigma` is ones."""
    syn = G.synthesis
    rows = _check_rows(rows, syn.num_layers)
    picked = [L.style.weight.detach().float() for L, row in style_groups(syn) if row in rows]
    A = picked[0].contiguous() if len(picked) == 1 else torch.cat(picked)
    M = ops.gram(A, row_norm=True, scale=1.0)
    evals, evecs, _ = ops.eigh_sym(M)
    return _result(evals, evecs, num, torch.ones_like(evals), None, "sefa", rows, None, None)


@torch.no_grad()
def pca_directions(G, samples=10000, seed=0, chunk=1000, num=None):
    """GANSpace's PCA in W: `samples` z from a CPU generator seeded with `seed`, mapped in chunks without truncation (the draws of
    infer.style_sigma); mean = the column means (dge_cols_mean_std); C = dge_gram(w, mean, 1 / samples); the eigenvectors of C by
    dge_eigh_sym.  sigma = sqrt(max(eigenvalue, 0)), the unit of an edit along the direction."""
    if samples < 1 or chunk < 1:
        raise ValueError("pca_directions: samples and chunk must be positive")
    dev = next(G.parameters()).device
    z = torch.randn(samples, G.z_space_dim, generator=torch.Generator().manual_seed(int(seed)))
    W = torch.empty((samples, G.synthesis.w_space_dim), dtype=torch.float32, device=dev)
    for i in range(0, samples, chunk):
        W[i:i + chunk] = G.mapping(z[i:i + chunk].to(dev))["w"].float()
    mean, _ = ops.cols_mean_std(W)
    Cm = ops.gram(W, mean=mean, scale=1.0 / samples)
    evals, evecs, _ = ops.eigh_sym(Cm)
    return _result(evals, evecs, num, torch.sqrt(torch.clamp(evals, min=0.0)), mean, "pca", list(range(G.synthesis.num_layers)),
                   int(samples), int(seed))


def save_directions(dirs, path):
    """The dict of sefa_directions / pca_directions -> `path` (directions.pt), tensors on the host."""
    missing = [k for k in KEYS if k not in dirs]
    if missing:
        raise ValueError(f"save_directions: the dict lacks {missing}")
    torch.save({k: (dirs[k].detach().cpu() if torch.is_tensor(dirs[k]) else dirs[k]) for k in KEYS}, path)


def load_directions(path):
    """directions.pt -> the dict, tensors on the host; ValueError for a file that is no such dict."""
    d = torch.load(path, map_location="cpu")
    if not isinstance(d, dict) or any(k not in d for k in KEYS):
        raise ValueError(f"load_directions: {path} is no directions file (a dict holding {', '.join(KEYS)})")
    K = d["directions"].shape[0]
    if d["directions"].dim() != 2 or d["eigenvalues"].numel() != K or d["sigma"].numel() != K:
        raise ValueError(f"load_directions: {path}: directions [K,D], eigenvalues [K] and sigma [K] do not agree")
    return d


def edit_direction(wp, dirs, k, amount, start=0, end=None):
    """wp [1,L,512] or [L,512] moved by `amount` sigmas along direction k of `dirs` in `end` W+ rows from row `start` (infer.edit_latent's
    arguments; end=None: every row from `start` on).  No arithmetic of its own: edit_latent(wp, direction k, amount * sigma[k])."""
    from .infer import edit_latent
    K = dirs["directions"].shape[0]
    if not 0 <= int(k) < K:
        raise ValueError(f"edit_direction: index {k} outside the {K} directions")
    L = wp.shape[-2]
    return edit_latent(wp, dirs["directions"][int(k):int(k) + 1], bonus=float(amount) * float(dirs["sigma"][int(k)]), start=start,
                       end=L - start if end is None else end)


# ------------------------------------------------------------------ CLI
def parse_rows(text):
    """`a-b` or `a` -> (a, b), a <= b"""
    try:
        a, _, b = text.partition("-")
        a, b = int(a), int(b) if b else int(a)
    except ValueError:
        raise SystemExit(f"directions: --rows takes `first-last` or one row, got {text!r}")
    if a > b:
        raise SystemExit(f"directions: --rows {text}: the first row is above the last")
    return a, b


def make_parser():
    from .models import add_model_args
    p = argparse.ArgumentParser(prog="dge_amd.directions", description="Semantic directions of StyleGAN2's W space: SeFa and W-space PCA")
    p.add_argument("command", choices=("fit", "apply"))
    add_model_args(p)
    p.set_defaults(mtype=2)
    p.add_argument("--method", choices=("sefa", "pca"), default="sefa")
    p.add_argument("--rows", default=None, help="W+ rows `first-last`: fit --method sefa: the blocks whose style weights enter; apply: the rows that move")
    p.add_argument("--num", type=int, default=None, help="fit: directions kept (default: all)")
    p.add_argument("--samples", type=int, default=10000, help="fit --method pca: mapped samples")
    p.add_argument("--seed", type=int, default=0, help="fit --method pca: seed of the z draws; also of a generator without checkpoint")
    p.add_argument("--directions", default=None, help="apply: the file `fit` wrote")
    p.add_argument("--wp", default=None, help="apply: a W+ code [1,L,512] (the projector's id{n}-wp.pt)")
    p.add_argument("--noise", default=None, help="apply: noise maps (the projector's id{n}-noise.pt)")
    p.add_argument("--index", type=int, default=0, help="apply: the direction")
    p.add_argument("--amounts", default="-3,-1.5,0,1.5,3", help="apply: the amounts in units of sigma, comma separated")
    p.add_argument("--out", default=None)
    return p


def parse_args(argv=None):
    p = make_parser()
    args = p.parse_args(argv)
    if args.mtype != 2:
        raise SystemExit("directions: --mtype must be 2 (StyleGAN2): StyleGAN1, PGGAN and BigGAN are not offered")
    if several_processes(env=True):
        raise SystemExit("directions: runs in one process (WORLD_SIZE > 1 is not supported)")
    if not args.out:
        raise SystemExit("directions: --out is required")
    size = args.img_size
    if size < 8 or size & (size - 1):
        raise SystemExit(f"directions: --img_size {size} is no power of two >= 8")
    args.num_layers = 2 * int(math.log2(size)) - 2
    args.row_range = None
    if args.rows is not None:
        a, b = args.row_range = parse_rows(args.rows)
        if a < 0 or b >= args.num_layers:
            raise SystemExit(f"directions: --rows {args.rows} outside the {args.num_layers} rows (0 .. {args.num_layers - 1}) of the model's W+ code")
    if args.command == "fit":
        if args.num is not None and args.num < 1:
            raise SystemExit("directions: --num must be positive")
        if args.method == "pca" and args.samples < 1:
            raise SystemExit("directions: --samples must be positive")
        if args.method == "pca" and args.rows is not None:
            raise SystemExit("directions: --rows belongs to --method sefa (the PCA is of W itself)")
    else:
        if not args.directions or not args.wp:
            raise SystemExit("directions: apply needs --directions and --wp")
        try:
            args.amount_list = [float(a) for a in args.amounts.split(",")]
        except ValueError:
            raise SystemExit(f"directions: --amounts takes comma-separated numbers, got {args.amounts!r}")
        args.dirs = load_directions(args.directions)
        K = args.dirs["directions"].shape[0]
        if not 0 <= args.index < K:
            raise SystemExit(f"directions: --index {args.index} outside the {K} directions of {args.directions}")
    return args


def _generator(args, dev):
    from .embedding_v2 import load_generator_smooth
    from .stylegan2_generator import StyleGAN2Generator
    torch.manual_seed(args.seed)
    kw = {k: getattr(args, k) for k in ("fmaps_base", "fmaps_max") if getattr(args, k) is not None}
    G = StyleGAN2Generator(args.img_size, compute_dtype=args.compute_dtype, **kw).to(dev)
    G.eval()
    if args.checkpoint_dir_GAN:
        load_generator_smooth(G, args.checkpoint_dir_GAN)
    return G


@torch.no_grad()
def main(argv=None):
    from .infer import save_image_grid
    args = parse_args(argv)
    dev = "cuda"
    G = _generator(args, dev)
    L = G.synthesis.num_layers
    if args.command == "fit":
        if args.method == "sefa":
            rows = None if args.row_range is None else range(args.row_range[0], args.row_range[1] + 1)
            dirs = sefa_directions(G, rows=rows, num=args.num)
        else:
            dirs = pca_directions(G, samples=args.samples, seed=args.seed, num=args.num)
        save_directions(dirs, args.out)
        print(args.out)
        return dirs
    wp = torch.load(args.wp, map_location="cpu").float()
    if wp.dim() == 2:
        wp = wp[None]
    if tuple(wp.shape) != (1, L, G.synthesis.w_space_dim):
        raise SystemExit(f"directions: --wp {args.wp} holds {tuple(wp.shape)}, the model's code is {(1, L, G.synthesis.w_space_dim)}")
    start, last = (0, L - 1) if args.row_range is None else args.row_range
    noises = [m.to(dev) for m in torch.load(args.noise, map_location="cpu")] if args.noise else None
    imgs = []
    for amount in args.amount_list:
        code = edit_direction(wp.to(dev), args.dirs, args.index, amount, start=start, end=last - start + 1)
        imgs.append(G.synthesis(code, randomize_noise=False, noises=noises)["image"].float())
    imgs = torch.cat(imgs)
    save_image_grid(imgs, args.out, nrow=imgs.shape[0])
    print(args.out)
    return imgs


if __name__ == "__main__":
    main()
