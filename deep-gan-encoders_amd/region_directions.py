"""Region directions of StyleGAN2 (ReSeFa: Zhu et al., Region-Based Semantic Factorization in GANs, ICML 2022), restated from the
publication: directions of W that edit the masked region of an inverted image and leave the rest alone.

With J the Jacobian of the (pooled) image with respect to the moved W+ rows at the code, along the axes of an orthonormal basis Q
[K,512], and mu the pooled mask, M_f = sum_n mu_n J_n J_n^T and M_b = sum_n (1 - mu_n) J_n J_n^T.  The directions are the
generalised eigenvectors that maximise v^T M_f v / (v^T M_b v + eps |v|^2), eps = reg * tr(M_b) / K.

* `jacobian_grams`    - X [K,N] by central differences (step h): per group of batch / 2 axes one dge_wp_axis_pairs, one synthesis of
                        `batch` images and one dge_fd_pool_diff into the group's rows of X; then one dge_gram_cols reads X once for
                        both Grams.  The mask is pooled with ops.area_pool.  N = 3 * jac_res^2.
* `solve_region`      - (beta, U) = dge_eigh_sym(M_b); S = diag((max(beta, 0) + eps)^-1/2) U; C = S M_f S^T (dge_matmul_f64acc);
                        (lambda, Y) = dge_eigh_sym(C); coefficient vectors c_k = normalise(y_k S).
* `region_directions` - the Grams averaged over the (code, mask) pairs, the solve, d_k = normalise(c_k Q) with the component of
                        largest magnitude positive; the dict of dge_amd.directions (method "region", sigma ones, eigenvalues = ratio)
                        plus ratio, fg_k = c_k M_f c_k^T, bg_k = c_k M_b c_k^T, coeffs, reg, step, jac_res, images.
* `edit_leakage`      - the measured counterpart of fg_k / bg_k: the mask-weighted and complement-weighted sums of squares of
                        pool(I(+amount)) - pool(I(-amount)) along direction k, with the same two kernels at K = 1.

Finite differences want f32 images: in bf16 the difference of two images is rounding noise divided by 2h.  `reg` = 1e-3 and
`step` = 0.25 are untuned defaults.  X holds K * 3 * jac_res^2 floats: 6.4 GB at K = 512 and jac_res = 1024.

Command line (`python -m dge_amd.region_directions`, the model flags of models.add_model_args, --compute_dtype f32 by default):

    fit   --wp a.pt [b.pt ...] --mask_dir DIR|m.pt [--noise a.pt ...] [--rows a-b] [--basis dirs.pt --basis_num K] [--step h]
          [--jac_res r] [--reg x] [--num n] [--batch B] --out region.pt
    check --directions region.pt --wp ... --mask_dir ... [--noise ...] [--amounts 1,2] [--jac_res r]

`fit` prints one line per kept direction (index, ratio, fg, bg) and writes region.pt, which `python -m dge_amd.directions apply
--directions region.pt ...` renders; `check` prints edit_leakage per direction and amount.

A lower module: it never imports the training script.
"""
import argparse
import math

import numpy as np
import torch

from . import ops
from .directions import KEYS, _check_rows, _generator, load_directions, parse_rows
from .embed_step import several_processes

EXTRA_KEYS = ("ratio", "fg", "bg", "coeffs", "reg", "step", "jac_res", "images")
MAX_AXES = 1024


def _row_range(rows, num_layers):
    """`rows` (None: all; else consecutive W+ rows, e.g. range(r0, r1)) -> (r0, r1); ValueError for rows outside the model or with a gap."""
    rows = _check_rows(rows, num_layers)
    if rows != list(range(rows[0], rows[-1] + 1)):
        raise ValueError(f"region_directions: rows {rows} are not one range of consecutive W+ rows")
    return rows[0], rows[-1] + 1


def _pool_factor(H, jac_res):
    """the pooling factor s = H / jac_res (default jac_res = min(H, 256)); ValueError unless jac_res is a power-of-two divisor of H"""
    r = min(H, 256) if jac_res is None else int(jac_res)
    if r < 1 or r > H or H % r or (H // r) & (H // r - 1) or r & (r - 1):
        raise ValueError(f"region_directions: jac_res = {jac_res} is no power-of-two divisor of the image size {H}")
    return H // r, r


def _code(wp, L, D):
    wp = wp.detach().float()
    if wp.dim() == 3 and wp.shape[0] == 1:
        wp = wp[0]
    if tuple(wp.shape) != (L, D):
        raise ValueError(f"region_directions: a code holds {tuple(wp.shape)}, the model's code is {(1, L, D)}")
    return wp.contiguous()


def _mask(mask, H, dev):
    mask = mask.detach().float()
    if mask.dim() == 3:
        mask = mask[None]
    if tuple(mask.shape) != (1, 1, H, H):
        raise ValueError(f"region_directions: a mask holds {tuple(mask.shape)}, the image is {(1, 1, H, H)}")
    return mask.to(dev).contiguous()


def check_basis(basis, D=512, tol=1e-4):
    """basis [K,D], K <= 1024, rows orthonormal within `tol` (max |Q Q^T - I|, by dge_matmul_f64acc) -> the f32 device matrix"""
    if basis.dim() != 2 or basis.shape[1] != D or basis.shape[0] < 1:
        raise ValueError(f"region_directions: the basis holds {tuple(basis.shape)}, expected [K,{D}]")
    if basis.shape[0] > MAX_AXES:
        raise ValueError(f"region_directions: K = {basis.shape[0]} axes, at most {MAX_AXES}")
    Q = basis.detach().float().contiguous()
    K = Q.shape[0]
    dev = float((ops.matmul_f64acc(Q, Q, trans_b=True) - torch.eye(K, device=Q.device)).abs().max())
    if not dev <= tol:
        raise ValueError(f"region_directions: the rows of the basis are not orthonormal: max |Q Q^T - I| = {dev:.3e} above {tol:g}")
    return Q


def _axes(basis, D, dev):
    if basis is None:
        return torch.eye(D, dtype=torch.float32, device=dev)
    return check_basis(basis.to(dev), D)


@torch.no_grad()
def _pooled_diffs(G, wp, Q, r0, r1, h, s, scale, noises, batch):
    """X [K, 3 (H/s)^2]: row k = scale * the s x s window sums of synthesis(wp + h q_k) - synthesis(wp - h q_k), batch / 2 axes per
    synthesis call"""
    syn = G.synthesis
    H, K = syn.resolution, Q.shape[0]
    N = 3 * (H // s) ** 2
    try:
        X = torch.empty((K, N), dtype=torch.float32, device=wp.device)
    except torch.cuda.OutOfMemoryError as e:
        raise RuntimeError(f"region_directions: the Jacobian operand of {K} x {N} floats ({4e-9 * K * N:.1f} GB) does not fit the device: "
                           f"lower --jac_res (now {H // s}) or --basis_num (now {K})") from e
    per = batch // 2
    for k0 in range(0, K, per):
        k1 = min(k0 + per, K)
        codes = ops.wp_axis_pairs(wp, Q[k0:k1], r0, r1, h)
        imgs = syn(codes, randomize_noise=False, noises=noises)["image"].float().contiguous()
        ops.fd_pool_diff(imgs, s, scale, X[k0:k1])
    return X


def _weights(mask, s):
    return (mask if s == 1 else ops.area_pool(mask, s)).reshape(-1)


@torch.no_grad()
def jacobian_grams(G, wp, mask, noises=None, rows=None, basis=None, step=0.25, jac_res=None, batch=8):
    """(M_f, M_b), each [K,K] f32 on the device, of the module docstring at the code wp [L,512] (or [1,L,512]) under mask [1,1,H,W]
    in [0,1] (white = the region).  noises: the maps of id{n}-noise.pt; rows: consecutive W+ rows that move (default all); basis
    [K,512] orthonormal rows (default the 512 unit vectors); jac_res: the resolution the images are pooled to (default min(H, 256))."""
    syn = G.synthesis
    dev = next(G.parameters()).device
    if not step > 0:
        raise ValueError(f"region_directions: step = {step} must be positive")
    if batch < 2 or batch % 2:
        raise ValueError(f"region_directions: batch = {batch} must be even (the images go through in pairs)")
    r0, r1 = _row_range(rows, syn.num_layers)
    s, _ = _pool_factor(syn.resolution, jac_res)
    wp = _code(wp, syn.num_layers, syn.w_space_dim).to(dev)
    mask = _mask(mask, syn.resolution, dev)
    Q = _axes(basis, syn.w_space_dim, dev)
    scale = float(np.float32(1.0 / (2.0 * float(step) * s * s)))
    X = _pooled_diffs(G, wp, Q, r0, r1, float(step), s, scale, noises, batch)
    return ops.gram_cols(X, wgt=_weights(mask, s), scale=1.0)


def region_eps(M_f, M_b, reg):
    """eps = reg * tr(M_b) / K, or reg * tr(M_f) / K where tr(M_b) = 0 (traces summed in float64); ValueError when both are 0"""
    K = M_b.shape[0]
    tb, tf = float(torch.diagonal(M_b).double().sum()), float(torch.diagonal(M_f).double().sum())
    if tb == 0.0 and tf == 0.0:
        raise ValueError("region_directions: both Gram matrices have trace 0 (the images do not move along any axis): nothing to solve")
    return float(reg) * (tb if tb != 0.0 else tf) / K


def _unit_rows(a):
    a64 = a.double()
    return (a64 / a64.norm(dim=1, keepdim=True)).float()


@torch.no_grad()
def solve_region(M_f, M_b, reg=1e-3):
    """The generalised symmetric eigenproblem of the module docstring on the device -> (ratio [K] descending, coeffs [K,K] with the
    unit coefficient vector c_k in row k)."""
    if not reg > 0:
        raise ValueError(f"region_directions: reg = {reg} must be positive")
    if M_f.dim() != 2 or M_f.shape != M_b.shape or M_f.shape[0] != M_f.shape[1]:
        raise ValueError(f"region_directions: M_f {tuple(M_f.shape)} and M_b {tuple(M_b.shape)} must be square and alike")
    eps = region_eps(M_f, M_b, reg)
    beta, U, _ = ops.eigh_sym(M_b)
    S = ((beta.double().clamp(min=0.0) + eps).rsqrt()[:, None] * U.double()).float().contiguous()
    Cm = ops.matmul_f64acc(ops.matmul_f64acc(S, M_f), S, trans_b=True)          # eigh_sym reads its upper triangle only
    lam, Y, _ = ops.eigh_sym(Cm)
    return lam, _unit_rows(ops.matmul_f64acc(Y, S))


def _largest_positive(d, *others):
    """rows of d with their component of largest magnitude (the first of equal ones) positive; the same signs to `others`"""
    top = d.abs().argmax(dim=1, keepdim=True)
    sign = torch.where(d.gather(1, top) < 0, -1.0, 1.0).to(d.dtype)
    return (d * sign, *(o * sign for o in others))


def _quad(c, M):
    """c_k M c_k^T per row (the product by dge_matmul_f64acc, the row sums in float64)"""
    return (ops.matmul_f64acc(c, M).double() * c.double()).sum(dim=1).float()


@torch.no_grad()
def region_directions(G, wps, masks, noises=None, rows=None, basis=None, step=0.25, jac_res=None, reg=1e-3, num=None, batch=8):
    """wps: codes [L,512] / [1,L,512]; masks: one [1,1,H,W] per code; noises: None or one list of maps per code.  The Grams are
    the arithmetic means over the pairs.  Returns the dict of the module docstring with `num` directions (default all K)."""
    wps, masks = list(wps), list(masks)
    noises = [None] * len(wps) if noises is None else list(noises)
    if not wps or len(masks) != len(wps) or len(noises) != len(wps):
        raise ValueError(f"region_directions: {len(wps)} codes, {len(masks)} masks and {len(noises)} sets of noise maps: one of each per image")
    syn = G.synthesis
    dev = next(G.parameters()).device
    r0, r1 = _row_range(rows, syn.num_layers)
    _, r = _pool_factor(syn.resolution, jac_res)
    Q = None if basis is None else check_basis(basis.to(dev), syn.w_space_dim)
    M_f = M_b = None
    for wp, mask, nz in zip(wps, masks, noises):
        f, b = jacobian_grams(G, wp, mask, noises=nz, rows=range(r0, r1), basis=Q, step=step, jac_res=r, batch=batch)
        M_f, M_b = (f, b) if M_f is None else (M_f + f, M_b + b)
    if len(wps) > 1:
        M_f, M_b = M_f / len(wps), M_b / len(wps)
    ratio, c = solve_region(M_f, M_b, reg=reg)
    d = c if Q is None else _unit_rows(ops.matmul_f64acc(c, Q))
    d, c = _largest_positive(d, c)
    K = ratio.numel()
    n = K if num is None else int(num)
    if not 1 <= n <= K:
        raise ValueError(f"region_directions: num = {num} outside 1 .. {K}")
    fg, bg = _quad(c, M_f), _quad(c, M_b)
    cut = lambda t: t[:n].contiguous()
    return dict(directions=cut(d), eigenvalues=cut(ratio), sigma=torch.ones(n, dtype=torch.float32, device=dev), mean=None, method="region",
                rows=list(range(r0, r1)), samples=None, seed=None, ratio=cut(ratio), fg=cut(fg), bg=cut(bg), coeffs=cut(c), reg=float(reg),
                step=float(step), jac_res=r, images=len(wps), M_f=M_f, M_b=M_b)


@torch.no_grad()
def edit_leakage(G, wp, mask, dirs, k, amount, noises=None, rows=None, jac_res=None):
    """(fg, bg): the mask-weighted and the complement-weighted sum of squares of pool(I(wp + amount d_k)) - pool(I(wp - amount d_k)),
    d_k = direction k of `dirs`, moved on `rows` (default: the rows of `dirs`), pooled to jac_res (default: that of `dirs`, else
    min(H, 256)).  The kernels of jacobian_grams at K = 1."""
    syn = G.synthesis
    dev = next(G.parameters()).device
    K = dirs["directions"].shape[0]
    if not 0 <= int(k) < K:
        raise ValueError(f"edit_leakage: index {k} outside the {K} directions")
    if not amount > 0:
        raise ValueError(f"edit_leakage: amount = {amount} must be positive")
    r0, r1 = _row_range(dirs["rows"] if rows is None else rows, syn.num_layers)
    s, _ = _pool_factor(syn.resolution, dirs.get("jac_res") if jac_res is None else jac_res)
    wp = _code(wp, syn.num_layers, syn.w_space_dim).to(dev)
    mask = _mask(mask, syn.resolution, dev)
    q = dirs["directions"][int(k):int(k) + 1].detach().float().to(dev).contiguous()
    X = _pooled_diffs(G, wp, q, r0, r1, float(amount), s, float(np.float32(1.0 / (s * s))), noises, 2)
    fg, bg = ops.gram_cols(X, wgt=_weights(mask, s), scale=1.0)
    return float(fg), float(bg)


def save_region(dirs, path):
    """The dict of region_directions -> `path`: the keys of a directions file and the region's own, tensors on the host
    (directions.load_directions reads it: extra keys are allowed)."""
    missing = [k for k in KEYS + EXTRA_KEYS if k not in dirs]
    if missing:
        raise ValueError(f"save_region: the dict lacks {missing}")
    torch.save({k: (dirs[k].detach().cpu() if torch.is_tensor(dirs[k]) else dirs[k]) for k in KEYS + EXTRA_KEYS}, path)


# ------------------------------------------------------------------ CLI
def make_parser():
    from .models import add_model_args
    p = argparse.ArgumentParser(prog="dge_amd.region_directions", description="Region directions of StyleGAN2's W space (ReSeFa)")
    p.add_argument("command", choices=("fit", "check"))
    add_model_args(p)
    p.set_defaults(mtype=2, compute_dtype="f32")
    p.add_argument("--wp", nargs="+", default=None, help="W+ codes [1,L,512] (the projector's id{n}-wp.pt), one per image")
    p.add_argument("--mask_dir", default=None, help="one mask per code: a directory (sorted-name order, white = the region) or a .pt tensor")
    p.add_argument("--noise", nargs="+", default=None, help="noise maps (the projector's id{n}-noise.pt), one file per code")
    p.add_argument("--rows", default=None, help="the W+ rows that move, `first-last` (default: all; check: the rows of the file)")
    p.add_argument("--basis", default=None, help="fit: a directions file whose first --basis_num rows span the search space (default: all of W)")
    p.add_argument("--basis_num", type=int, default=None, help="fit: rows of --basis taken (default: all)")
    p.add_argument("--step", type=float, default=0.25, help="fit: the finite-difference step h (an untuned default)")
    p.add_argument("--jac_res", type=int, default=None, help="the resolution the images are pooled to (default min(img_size, 256))")
    p.add_argument("--reg", type=float, default=1e-3, help="fit: eps = reg * tr(M_b) / K (an untuned default)")
    p.add_argument("--num", type=int, default=None, help="fit: directions kept (default: all)")
    p.add_argument("--batch", type=int, default=8, help="fit: images per synthesis call (even)")
    p.add_argument("--seed", type=int, default=0, help="seed of a generator without checkpoint")
    p.add_argument("--directions", default=None, help="check: the file `fit` wrote")
    p.add_argument("--amounts", default="1,2", help="check: the amounts, comma separated")
    p.add_argument("--out", default=None)
    return p


def parse_args(argv=None):
    args = make_parser().parse_args(argv)
    die = lambda msg: SystemExit("region_directions: " + msg)
    if args.mtype != 2:
        raise die("--mtype must be 2 (StyleGAN2): StyleGAN1, PGGAN and BigGAN are not offered")
    if several_processes(env=True):
        raise die("runs in one process (WORLD_SIZE > 1 is not supported)")
    size = args.img_size
    if size < 8 or size & (size - 1):
        raise die(f"--img_size {size} is no power of two >= 8")
    args.num_layers = 2 * int(math.log2(size)) - 2
    if not args.wp or not args.mask_dir:
        raise die("--wp and --mask_dir are required")
    if args.noise is not None and len(args.noise) != len(args.wp):
        raise die(f"--noise names {len(args.noise)} files, --wp {len(args.wp)}: one set of maps per code")
    try:
        _pool_factor(size, args.jac_res)
    except ValueError:
        raise die(f"--jac_res {args.jac_res} is no power-of-two divisor of --img_size {size}")
    args.row_range = None
    if args.rows is not None:
        a, b = args.row_range = parse_rows(args.rows)
        if a < 0 or b >= args.num_layers:
            raise die(f"--rows {args.rows} outside the {args.num_layers} rows (0 .. {args.num_layers - 1}) of the model's W+ code")
    if args.command == "fit":
        if not args.out:
            raise die("--out is required")
        if not args.step > 0:
            raise die(f"--step {args.step} must be positive")
        if not args.reg > 0:
            raise die(f"--reg {args.reg} must be positive")
        if args.batch < 2 or args.batch % 2:
            raise die(f"--batch {args.batch} must be even (the images go through in pairs)")
        if args.num is not None and args.num < 1:
            raise die("--num must be positive")
        if args.basis_num is not None and (args.basis is None or args.basis_num < 1):
            raise die("--basis_num belongs to --basis and must be positive")
        if args.basis_num is not None and args.basis_num > MAX_AXES:
            raise die(f"--basis_num {args.basis_num}: K > {MAX_AXES} axes")
    else:
        if not args.directions:
            raise die("check needs --directions")
        try:
            args.amount_list = [float(a) for a in args.amounts.split(",")]
        except ValueError:
            raise die(f"--amounts takes comma-separated numbers, got {args.amounts!r}")
        if any(not a > 0 for a in args.amount_list):
            raise die(f"--amounts {args.amounts}: every amount must be positive")
    return args


def _inputs(args, G, dev):
    """the codes, the masks and the noise maps of the command line"""
    from .projector import load_masks
    syn = G.synthesis
    shape = (1, syn.num_layers, syn.w_space_dim)
    wps = []
    for path in args.wp:
        wp = torch.load(path, map_location="cpu").float()
        wp = wp[None] if wp.dim() == 2 else wp
        if tuple(wp.shape) != shape:
            raise SystemExit(f"region_directions: --wp {path} holds {tuple(wp.shape)}, the model's code is {shape}")
        wps.append(wp.to(dev))
    try:
        masks = load_masks(args.mask_dir, syn.resolution, len(wps))
    except SystemExit as e:
        raise SystemExit(str(e).replace("projector:", "region_directions:").replace("--img_dir", "--wp"))
    masks = [masks[i:i + 1].to(dev) for i in range(len(wps))]
    noises = None
    if args.noise:
        noises = [[m.to(dev) for m in torch.load(path, map_location="cpu")] for path in args.noise]
    return wps, masks, noises


@torch.no_grad()
def main(argv=None):
    args = parse_args(argv)
    dev = "cuda"
    G = _generator(args, dev)
    wps, masks, noises = _inputs(args, G, dev)
    rows = None if args.row_range is None else range(args.row_range[0], args.row_range[1] + 1)
    if args.command == "fit":
        basis = None
        if args.basis:
            basis = load_directions(args.basis)["directions"].float()
            if args.basis_num is not None:
                if args.basis_num > basis.shape[0]:
                    raise SystemExit(f"region_directions: --basis_num {args.basis_num} above the {basis.shape[0]} directions of {args.basis}")
                basis = basis[:args.basis_num]
        try:
            dirs = region_directions(G, wps, masks, noises=noises, rows=rows, basis=basis, step=args.step, jac_res=args.jac_res, reg=args.reg,
                                     num=args.num, batch=args.batch)
        except (ValueError, RuntimeError) as e:
            if not str(e).startswith("region_directions:"):
                raise
            raise SystemExit(str(e))
        save_region(dirs, args.out)
        for k, (lam, fg, bg) in enumerate(zip(dirs["ratio"].tolist(), dirs["fg"].tolist(), dirs["bg"].tolist())):
            print(f"{k:4d}  ratio {lam:.6e}  fg {fg:.6e}  bg {bg:.6e}")
        print(args.out)
        return dirs
    dirs = load_directions(args.directions)
    out = []
    for i, (wp, mask) in enumerate(zip(wps, masks)):
        for k in range(dirs["directions"].shape[0]):
            for amount in args.amount_list:
                try:
                    fg, bg = edit_leakage(G, wp, mask, dirs, k, amount, noises=None if noises is None else noises[i], rows=rows,
                                          jac_res=args.jac_res)
                except ValueError as e:
                    raise SystemExit(str(e))
                out.append((i, k, amount, fg, bg))
                print(f"image {i}  direction {k:4d}  amount {amount:g}  fg {fg:.6e}  bg {bg:.6e}")
    return out


if __name__ == "__main__":
    main()
