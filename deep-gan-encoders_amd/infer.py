"""Inference-side helpers of the reference on the HIP path (thin wrappers over the same forward kernels):

* `reconstruct`   - inferE.py:101-141 / rec_real_img.py / synthesized_IMG.py: G(z) -> E -> G(w2) once, no gradients;
* `edit_latent`   - embeded_img_edit.py:28-41: w[start:start+end] = (w + bonus*direction)[start:start+end] on a W+ code,
                    then one Gs.forward(w, lod); directions for StyleGAN2, which ships no boundary file, come from
                    `dge_amd.directions` (SeFa, W-space PCA), whose `edit_direction` calls this function;
* `style_sigma` / `edit_styles` - StyleSpace edits ("block, channel, + k sigma") on the per-channel style codes of StyleGAN2
                    (style_codes.StyleCodes.rows, `id{n}-s.pt`): no boundary file is needed;
* `image_metrics` - comparing-baseline.py:21-45 on device: PSNR / MSE on [0,255], cosine on [-1,1], LPIPS and the skimage SSIM of
                    that script (`ssim_skimage`: 7x7 uniform window, sample covariance, data_range 255 - a different statistic
                    from the training loss's pytorch_ssim, which `losses.space_loss` reports);
* `load_images` / `reconstruct_images` - rec_real_img.py:84-120: image files -> `[N,3,S,S]` batch in [-1,1] (PIL, the script's
                    Resize + ToTensor; `training_utils.imgPath2loader` with `bicubic=True`) -> E -> G, the "invert this image" path;
* `save_image`    - torchvision.utils.save_image(img*0.5+0.5, path) for a single image batch laid out in one row;
* `quantize_u8` / `image_metrics_rows` - the numbers of comparing-baseline.py:46-87: every image pair on its own, on the 8-bit
                    images a saved file holds (exact integer sums, f64 metrics; ops.image_metrics_u8);
* `MetricsTable`  - the per-pair table behind `<out>/metrics.csv` / `metrics.json` of `infer eval`, `rec --metrics` and
                    `python -m dge_amd.compare`.
"""
import math

import torch

from . import ops
from ._lib import lib, check
from .generators import set_seed
from .losses import batch_sums
from .models import add_model_args, load_models
from .train_step import TrainStep
from .ops import _f32, _p, _stream


@torch.no_grad()
def reconstruct(step, z=None, iteration=4, noises=None):
    """One inversion round trip with the models of a training step (`TrainStep`, any --mtype): returns dict(imgs1, w1, const2, w2, imgs2).
    `noises`: optional encoder noise tensors (the reference draws them on the CPU, model/E/E.py:60,73 - parity runs inject them)."""
    gen, E, B = step.gen, step.E, step.batch_size
    if z is None:
        set_seed(iteration)                                   # inferE.py:101-103 (seed 4)
        z = gen.draw(iteration, B, step.z_dim)
    z = z.to(step.dev)
    imgs1, w1 = gen.sample(z)
    const2, w2 = gen.encode(E, imgs1, noises)
    return dict(imgs1=imgs1, w1=w1, const2=const2, w2=w2, imgs2=gen.synth(w2))


def load_images(paths, size, bicubic=False, device="cuda"):
    """rec_real_img.py:84-98: Image.open(p).convert('RGB') -> Resize((size, size)) (PIL bilinear, what torchvision's Resize does
    to a PIL image) -> ToTensor ([0,1], CHW) -> stacked, then the script's `* 2 - 1` (:101).  bicubic=True is
    training_utils.imgPath2loader (:11-15: `image.resize((size, size))`, PIL's default filter).  Host-side file I/O."""
    import numpy as np
    from PIL import Image
    out = []
    for p in paths:
        img = Image.open(p).convert("RGB")
        img = img.resize((size, size)) if bicubic else img.resize((size, size), Image.BILINEAR)
        out.append(torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255.0))
    return (torch.stack(out, dim=0) * 2 - 1).to(device)


@torch.no_grad()
def reconstruct_images(step, imgs1):
    """rec_real_img.py:100-112: real images [N,3,S,S] in [-1,1] -> E -> G, one image at a time as the script does (the
    encoder's instance statistics are per sample, so batching changes nothing but the noise draws).  Returns (w2, imgs2)."""
    gen, E = step.gen, step.E
    if gen.conditional:
        raise ValueError("BigGAN needs the class-conditional vector of the image (rec_real_img.py:104); use E(img, cond) directly")
    ws, outs = [], []
    for j in imgs1:
        _, w2 = E(j.unsqueeze(0))
        ws.append(w2)
        outs.append(gen.synth(w2))
    return torch.cat(ws), torch.cat(outs)


def edit_latent(w, direction, bonus=70.0, start=0, end=3):
    """embeded_img_edit.py:28-41.  w: [1,L,512] or [L,512] W+ code, direction: [1,512] (InterfaceGAN boundary).  Rows
    start .. start+end-1 move along the direction, the others keep the identity features.  Returns [1,L,512]."""
    w2 = w.detach().clone().float()
    w2 = w2.squeeze(0) if w2.dim() == 3 else w2
    d = torch.as_tensor(direction).float().to(w2.device).expand(w2.shape[0], w2.shape[1])
    w2[start:start + end] = (w2 + bonus * d)[start:start + end]
    return w2.reshape(1, w2.shape[0], w2.shape[1])


def style_block_names(nblocks):
    """The names of the `nblocks` = (L - 1) + L / 2 blocks of a StyleSpace code in file order: layer0 .. layer{L-2}, output0 .. output{L/2-1}."""
    nl = (2 * nblocks + 2) // 3
    if nblocks < 2 or nl % 2 or (nl - 1) + nl // 2 != nblocks:
        raise ValueError(f"{nblocks} blocks are not the StyleSpace code of a StyleGAN2 synthesis network ((L - 1) conv + L / 2 toRGB blocks)")
    return [f"layer{i}" for i in range(nl - 1)] + [f"output{k}" for k in range(nl // 2)]


@torch.no_grad()
def style_sigma(G, samples=10000, seed=0, chunk=1000):
    """(mean, sigma) of the StyleSpace codes of `samples` z drawn from a CPU generator seeded with `seed` and mapped without
    truncation: two lists in block order (style_codes.StyleCodes.names), one [C_g] tensor per block.  The styles of a chunk are
    written into the matrix [samples, sum C_g], and dge_cols_mean_std takes the columns: sigma = sqrt(sum (s - mean)^2 / samples),
    the unit of `edit_styles`."""
    from .autograd_s2 import styles_from_wp
    from .style_codes import style_layout
    if samples < 1 or chunk < 1:
        raise ValueError("style_sigma: samples and chunk must be positive")
    dev = next(G.parameters()).device
    syn = G.synthesis
    _, channels, _, per_row = style_layout(syn, 1)
    z = torch.randn(samples, G.z_space_dim, generator=torch.Generator().manual_seed(int(seed)))
    X = torch.empty((samples, per_row), dtype=torch.float32, device=dev)
    for i in range(0, samples, chunk):
        w = G.mapping(z[i:i + chunk].to(dev))["w"].float().contiguous()
        n = w.shape[0]
        flat = styles_from_wp(syn, ops.w_broadcast(w, syn.num_layers))
        off = 0
        for C in channels:          # block g of the chunk [n,C_g] sits at n * off_g: to the columns off_g .. of the chunk's rows
            X[i:i + n, off:off + C] = flat[n * off:n * (off + C)].view(n, C)
            off += C
    mean, std = ops.cols_mean_std(X)
    return list(mean.split(channels)), list(std.split(channels))


def edit_styles(rows, block, channel, amount, sigma=None):
    """A StyleSpace edit "block, channel, + amount": `rows` is the code of one image, the list of [1,C_g] tensors of `id{n}-s.pt`
    (StyleCodes.rows); `block` a name (`layer9`, `output3`) or an index; `amount` is added to that channel, times
    sigma[block][channel] where `sigma` (style_sigma's second list) is given.  Returns new rows; plain tensor arithmetic, on
    whatever device the rows are."""
    rows = list(rows)
    names = style_block_names(len(rows))
    if isinstance(block, str):
        if block not in names:
            raise ValueError(f"edit_styles: no block {block!r}; the blocks are {names[0]} .. {names[-1]}")
        g = names.index(block)
    else:
        g = int(block)
        if not 0 <= g < len(rows):
            raise ValueError(f"edit_styles: block index {block} outside the {len(rows)} blocks")
    C = rows[g].shape[-1]
    if not 0 <= int(channel) < C:
        raise ValueError(f"edit_styles: channel {channel} outside the {C} channels of {names[g]}")
    if sigma is not None and (len(sigma) != len(rows) or sigma[g].numel() != C):
        raise ValueError("edit_styles: sigma holds one [C_g] tensor per block (style_sigma)")
    unit = 1.0 if sigma is None else float(sigma[g].reshape(-1)[int(channel)])
    out = [r.detach().clone() for r in rows]
    out[g][..., int(channel)] += float(amount) * unit
    return out


@torch.no_grad()
def image_metrics(img1, img2, lpips_model=None):
    """img1, img2: [B,3,H,W] in [-1,1] on the GPU -> dict of device scalars: psnr / mse on the [0,255] scale, cosine on
    [-1,1], lpips (mean over the batch) when a model is given.  One reduction pass (dge_loss_reduce)."""
    a = img1.detach().float().contiguous()
    b = img2.detach().float().contiguous()
    s = batch_sums(a, b, (0, 0, a.shape[2], a.shape[3]))
    n = float(a.numel())
    mse255 = s[0] / n * (127.5 * 127.5)                      # x255 = (x + 1) * 127.5
    out = dict(mse=mse255, psnr=10.0 * torch.log10(255.0 * 255.0 / mse255), cosine=s[1] / torch.sqrt(s[2] * s[3]))
    out["ssim"] = ssim_skimage(a, b).mean()
    if lpips_model is not None:
        out["lpips"], _ = lpips_model.value_and_grad(a, b, need_grad=False)
    return out


@torch.no_grad()
def ssim_skimage(img1, img2):
    """skimage.measure.compare_ssim(x, y, data_range=255, multichannel=True) of comparing-baseline.py:25 for every image pair of
    a batch: img1, img2 [B,C,H,W] in [-1,1] on the GPU (taken to the script's [0,255] scale inside the kernel) -> [B]."""
    a = img1.detach().float().contiguous()
    b = img2.detach().float().contiguous()
    B, Cc, H, W = a.shape
    if H < 7 or W < 7:
        raise ValueError("win_size exceeds image extent (skimage raises the same for images smaller than 7x7)")
    sums = torch.zeros(B * Cc, dtype=torch.float32, device=a.device)
    check(lib().dge_ssim_box7(_f32(a), _f32(b), _p(sums), B * Cc, H, W, 127.5, 127.5, 255.0, _stream()), "dge_ssim_box7")
    return sums.view(B, Cc).sum(1) / float(Cc * (H - 6) * (W - 6))


@torch.no_grad()
def quantize_u8(img):
    """img [B,C,H,W] f32 or bf16 in [-1,1] on the GPU -> device uint8 [B,H,W,C]: the bytes `save_image_grid` /
    torchvision.utils.save_image write for it (PIL's layout), rounded on the device with the host formula's f32 arithmetic."""
    return ops.quantize_u8(img.detach().contiguous())


@torch.no_grad()
def minmax_unit(x):
    """(x - min x) / (max x - min x) over the whole float32 device tensor: the guided-gradient picture of the mis-align scripts
    (E_mis_align_cropping_s1.py:292-293, `grads -= np.max(np.min(grads), 0); grads /= np.max(grads)` - np.max's second argument is an
    axis, so the first line subtracts the global minimum).  Two launches (dge_minmax_unit), no host read; the minimum maps to exactly
    0 and the maximum to exactly 1.  A constant tensor divides by zero, as the script does."""
    x = x.detach().contiguous()
    y = torch.empty_like(x)
    n = x.numel()
    slots = torch.empty((lib().dge_minmax_unit_slots(n), 2), dtype=torch.float32, device=x.device)
    check(lib().dge_minmax_unit(_f32(x), _f32(y), n, _f32(slots), _stream()), "dge_minmax_unit")
    ops.log_kernel()
    return y


@torch.no_grad()
def image_metrics_rows(img1, img2, lpips_model=None, quantize=True):
    """comparing-baseline.py:67-87 for a batch: every pair (img1[i], img2[i]) measured on its own, on 8-bit images as the script
    reads them from files (ToTensor()*255).  Inputs: uint8 [B,H,W,3] (decoded files, `quantize_u8` output), or float [B,3,H,W] in
    [-1,1], which is quantised first - the numbers of the saved files.  Returns a dict of [B] float64 device tensors psnr, ssim,
    mse (on [0,255]), cosine (on [-1,1]), `isums` [B,5] int64 (sum a, sum b, sum a^2, sum b^2, sum ab) and, with a model, `lpips`
    [B] f32 on q/255*2-1.  PSNR is +inf for identical images (skimage).  One launch, no host sync.  The batch-coupled float
    statistics stay `image_metrics`; quantize=False on floats is refused."""
    q = []
    for t in (img1, img2):
        t = t.detach()
        if t.dtype == torch.uint8:
            q.append(t)
        elif t.is_floating_point():
            if not quantize:
                raise ValueError("image_metrics_rows measures 8-bit images: float inputs are quantised (quantize=True); the float, "
                                 "batch-coupled form is image_metrics")
            if t.dim() != 4 or t.shape[1] != 3:
                raise ValueError(f"image_metrics_rows: float images are [B,3,H,W] in [-1,1], got {tuple(t.shape)}")
            q.append(quantize_u8(t))
        else:
            raise ValueError(f"image_metrics_rows: uint8 [B,H,W,3] or float [B,3,H,W] images, got {t.dtype}")
    a, b = q
    if a.dim() != 4 or a.shape[3] != 3 or a.shape != b.shape:
        raise ValueError(f"image_metrics_rows: two image batches of one shape [B,H,W,3], got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.shape[1] < 7 or a.shape[2] < 7:
        raise ValueError("win_size exceeds image extent (skimage raises the same for images smaller than 7x7)")
    isums, _, m = ops.image_metrics_u8(a, b)
    out = dict(psnr=m[:, 0], ssim=m[:, 1], mse=m[:, 2], cosine=m[:, 3], isums=isums)
    if lpips_model is not None:
        fa, fb = (t.permute(0, 3, 1, 2).float().div(255.0).mul(2.0).sub(1.0).contiguous() for t in (a, b))
        out["lpips"], _ = lpips_model.value_and_grad(fa, fb, need_grad=False, per_sample=True)
    return out


METRIC_COLUMNS = ("psnr", "ssim", "mse", "lpips", "cosine")           # the order of comparing-baseline.py's progress line


class MetricsTable:
    """Per-pair metrics of a run, kept on the device until `write`: `add` takes the dict of `image_metrics_rows` and the two file
    names of every pair and makes no host read; `write` reads once and writes <out>/metrics.csv (one row per pair: index, file1,
    file2 and the five metrics, floats in repr form, the lpips column empty without a model) and <out>/metrics.json (the means
    the script prints at its end, `count`, `identical_pairs`; `lpips: null` without a model).  A pair with mse == 0 puts inf into
    the PSNR mean, as in the script, and is counted in `identical_pairs`."""

    def __init__(self):
        self.names, self.rows, self.lpips = [], [], []

    def add(self, m, names1, names2):
        self.names += list(zip(names1, names2))
        self.rows.append(torch.stack((m["psnr"], m["ssim"], m["mse"], m["cosine"]), dim=1))
        if "lpips" in m:
            self.lpips.append(m["lpips"].double())

    def values(self):
        """[(psnr, ssim, mse, lpips | None, cosine)] as Python floats: the one host read"""
        if not self.rows:
            return []
        rows = torch.cat(self.rows)
        if self.lpips:
            rows = torch.cat((rows, torch.cat(self.lpips).unsqueeze(1)), dim=1)
        rows = rows.cpu().tolist()
        return [(r[0], r[1], r[2], r[4] if len(r) > 4 else None, r[3]) for r in rows]

    def write(self, out_dir, progress=None):
        """`progress`: a callable taking the script's running-mean line of every pair (comparing-baseline.py:84-85)."""
        import json
        import os
        vals = self.values()
        os.makedirs(out_dir, exist_ok=True)
        sums = [0.0] * 5
        lines = ["index,file1,file2," + ",".join(METRIC_COLUMNS)]
        for i, ((n1, n2), v) in enumerate(zip(self.names, vals)):
            lines.append("%d,%s,%s,%s" % (i, n1, n2, ",".join("" if x is None else repr(x) for x in v)))
            sums = [s + (0.0 if x is None else x) for s, x in zip(sums, v)]
            if progress is not None:
                progress("img_num:%d--psnr:%f--ssim:%f--mse_value:%f--lpips_value:%f--cosine_value:%f" % ((i + 1,) + tuple(s / (i + 1) for s in sums)))
        n = len(vals)
        summary = dict(count=n, identical_pairs=sum(1 for v in vals if v[2] == 0.0))
        for k, name in enumerate(METRIC_COLUMNS):
            summary[name] = None if (n == 0 or vals[0][k] is None) else sums[k] / n
        paths = os.path.join(out_dir, "metrics.csv"), os.path.join(out_dir, "metrics.json")
        with open(paths[0], "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(paths[1], "w") as f:
            json.dump(summary, f, indent=1)                       # an infinite PSNR mean is written as Infinity (Python's json)
            f.write("\n")
        return list(paths)


def add_lpips_args(parser):
    parser.add_argument("--vgg_weights", default=None, help="torchvision vgg16 checkpoint (features.*) or an lpips.LPIPS state_dict")
    parser.add_argument("--lpips_weights", default=None, help="the lpips package's weights/v0.1/vgg.pth (lin{k}.model.1.weight)")
    parser.add_argument("--allow_standin_lpips", action="store_true", help="report LPIPS on seeded stand-in weights (NOT the published metric)")
    return parser


def lpips_from_args(args, device="cuda", compute_dtype="bf16"):
    """The LPIPS model of a metrics run, or None when none of --vgg_weights / --lpips_weights / --allow_standin_lpips is given
    (the lpips column then stays empty)."""
    from .lpips import LPIPS
    from .models import load_lpips_weights
    if not (args.vgg_weights or args.lpips_weights or args.allow_standin_lpips):
        return None
    torch.manual_seed(0)
    LP = LPIPS(compute_dtype=compute_dtype).to(device)
    LP.eval()
    return load_lpips_weights(LP, args.vgg_weights, args.lpips_weights, allow_standin=args.allow_standin_lpips)


def save_u8(q, path):
    """q [H,W,3] uint8 (one image of `quantize_u8`) -> PNG, the bytes as they are."""
    from PIL import Image
    Image.fromarray(q.cpu().numpy()).save(path)


def save_image(img, path):
    """img [B,3,H,W] in [-1,1] -> PNG (samples side by side)."""
    from PIL import Image
    x = (img.detach().float().cpu() * 0.5 + 0.5).clamp(0, 1)
    x = torch.cat(list(x), dim=2)                              # [3,H,B*W]
    Image.fromarray((x.permute(1, 2, 0) * 255.0 + 0.5).to(torch.uint8).numpy()).save(path)


def save_image_grid(imgs, path, nrow=10):
    """torchvision.utils.save_image(imgs*0.5+0.5, path, nrow=nrow) without torchvision: `nrow` images per row, 2 px padding."""
    from PIL import Image
    x = (imgs.detach().float().cpu() * 0.5 + 0.5).clamp(0, 1)
    n, c, h, w = x.shape
    cols = min(nrow, n)
    rows = (n + cols - 1) // cols
    pad = 2
    grid = torch.zeros(c, rows * (h + pad) + pad, cols * (w + pad) + pad)
    for i in range(n):
        r, q = divmod(i, cols)
        grid[:, pad + r * (h + pad):pad + r * (h + pad) + h, pad + q * (w + pad):pad + q * (w + pad) + w] = x[i]
    Image.fromarray((grid.permute(1, 2, 0) * 255.0 + 0.5).to(torch.uint8).numpy()).save(path)


def _step_from_args(args, device="cuda"):
    G, Gm, E, _ = load_models(args, device=device, lpips=False)
    G.eval()
    E.eval()
    return TrainStep(G, E, None, mapping=Gm, batch_size=args.batch_size, z_dim=args.z_dim)


def main(argv=None):
    """Entry points of the reference's inference scripts on the HIP path (`python -m dge_amd.infer <command> ...`), every
    --mtype and its checkpoint container (models.load_models):

    * `infer` - inferE.py:101-141: seed 4, z -> G -> E -> G, writes <out>/v2ep<seed>.png (originals over reconstructions);
    * `rec`   - rec_real_img.py:84-127: every image of --img_dir -> E -> G, writes <out>/real/%05d_realimg.png and
                <out>/rec/%05d_mtv_rec.png;
    * `synth` - synthesized_IMG.py:97-145: for iteration in 30000 .. 30000 + --iterations: set_seed(iteration), z -> G -> E -> G,
                writes <out>/id<flag>_%05d.png (nrow 10: originals then reconstructions);
    * `eval`  - the `synth` loop measured instead of drawn: imgs1 and imgs2 of every iteration are quantised to the 8-bit
                images a file would hold and every pair's PSNR / SSIM / MSE / cosine (LPIPS with the weight flags) is kept on
                the device (`image_metrics_rows`); one host read at the end writes <out>/metrics.csv and metrics.json
                (`MetricsTable`).  --dump_dir D also writes the quantised bytes as D/real/%05d.png and D/rec/%05d.png, on
                which `python -m dge_amd.compare` reproduces the table.
    `rec --metrics` adds the same two files for the real images against their reconstructions (the images without the
    2-pixel frame of the PNGs it writes)."""
    import argparse
    import os
    parser = argparse.ArgumentParser(prog="dge_amd.infer", description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("command", choices=("infer", "rec", "synth", "eval"))
    add_model_args(parser)
    parser.add_argument("--batch_size", type=int, default=5)
    parser.add_argument("--seed", type=int, default=4)
    parser.add_argument("--iterations", type=int, default=1)
    parser.add_argument("--img_dir", default=None, help="rec: directory of images (sorted by name)")
    parser.add_argument("--out", default="./result")
    parser.add_argument("--metrics", action="store_true", help="rec: also write <out>/metrics.csv and metrics.json")
    parser.add_argument("--dump_dir", default=None, help="eval: also write every pair as <dump_dir>/real/%%05d.png and rec/%%05d.png")
    add_lpips_args(parser)
    args = parser.parse_args(argv)
    os.makedirs(args.out, exist_ok=True)
    step = _step_from_args(args)
    written = []
    table = MetricsTable() if args.command == "eval" or (args.command == "rec" and args.metrics) else None
    LP = lpips_from_args(args, step.dev, args.compute_dtype) if table is not None else None
    if args.command == "infer":
        r = reconstruct(step, iteration=args.seed)
        path = os.path.join(args.out, "v2ep%d.png" % args.seed)
        save_image_grid(torch.cat((r["imgs1"][:args.batch_size], r["imgs2"][:args.batch_size])), path, nrow=args.batch_size)
        written.append(path)
    elif args.command == "rec":
        if not args.img_dir:
            parser.error("rec needs --img_dir")
        names = sorted(n for n in os.listdir(args.img_dir) if n.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")))
        if not names:
            parser.error("rec: no images in " + args.img_dir)
        d1, d2 = os.path.join(args.out, "real"), os.path.join(args.out, "rec")
        os.makedirs(d1, exist_ok=True)
        os.makedirs(d2, exist_ok=True)
        imgs = load_images([os.path.join(args.img_dir, n) for n in names], args.img_size, device=step.dev)
        set_seed(args.seed)                                   # the encoder draws noise in every forward (model/E/E.py:62,72)
        _, rec = reconstruct_images(step, imgs)
        for i in range(imgs.shape[0]):
            a, b = os.path.join(d1, "%s_realimg.png" % str(i).rjust(5, "0")), os.path.join(d2, "%s_mtv_rec.png" % str(i).rjust(5, "0"))
            save_image_grid(imgs[i:i + 1], a, nrow=1)
            save_image_grid(rec[i:i + 1], b, nrow=1)
            written += [a, b]
        if table is not None:
            table.add(image_metrics_rows(imgs, rec, LP), [os.path.basename(w) for w in written[0::2]], [os.path.basename(w) for w in written[1::2]])
    elif args.command == "eval":
        B = args.batch_size
        if args.dump_dir:
            os.makedirs(os.path.join(args.dump_dir, "real"), exist_ok=True)
            os.makedirs(os.path.join(args.dump_dir, "rec"), exist_ok=True)
        for iteration in range(30000, 30000 + args.iterations):
            r = reconstruct(step, iteration=iteration % 30000 if step.gen.conditional else iteration)
            q1, q2 = quantize_u8(r["imgs1"]), quantize_u8(r["imgs2"])
            names = ["%s.png" % str((iteration - 30000) * B + j).rjust(5, "0") for j in range(q1.shape[0])]
            table.add(image_metrics_rows(q1, q2, LP), names, names)
            if args.dump_dir:
                for j, n in enumerate(names):
                    for sub, q in (("real", q1), ("rec", q2)):
                        save_u8(q[j], os.path.join(args.dump_dir, sub, n))
                        written.append(os.path.join(args.dump_dir, sub, n))
    else:
        for iteration in range(30000, 30000 + args.iterations):
            r = reconstruct(step, iteration=iteration % 30000 if step.gen.conditional else iteration)
            flag = step.gen.flag
            path = os.path.join(args.out, "id%s_%s.png" % (flag, str(iteration - 30000).rjust(5, "0")))
            save_image_grid(torch.cat((r["imgs1"], r["imgs2"])), path, nrow=10)
            written.append(path)
    if table is not None:
        written += table.write(args.out)
    for w in written:
        print(w)
    return written


if __name__ == "__main__":
    main()
