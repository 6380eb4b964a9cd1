"""`python -m dge_amd.compare --dir1 A --dir2 B [--img_size S]`: the table the paper is judged by - the loop of the reference's
comparing-baseline.py:46-87 over a folder of originals and a folder of reconstructions, PSNR / SSIM / MSE / LPIPS / cosine of
every pair on the 8-bit images the files hold.

The files are decoded on the host (`.png` / `.jpg`, `convert("RGB")`, PIL-bilinear resize to --img_size when given: what
`infer.load_images` does); their bytes go to the device as uint8 and every group of --batch_size pairs is measured by one launch
(`infer.image_metrics_rows`), each pair on its own.  Per pair the script's running-mean line is printed; `<out>/metrics.csv`
holds one row per pair with the two file names, `<out>/metrics.json` the means and the count (`lpips: null` without weights).

Decisions where the script leaves room or goes wrong:

* pairs are formed in sorted name order, the k-th file of --dir1 with the k-th of --dir2 (the script zips two unsorted
  os.listdir results, so its pairing depends on the file system);
* folders with unequal numbers of images are refused with a message (zip would drop the surplus silently);
* without --img_size the two images of a pair must have equal sizes, else the run exits (the script resizes always); groups are
  cut where the size changes, so folders of mixed sizes work;
* a pair with mse == 0 contributes inf to the PSNR mean, as in the script (skimage returns inf), and is counted in
  `identical_pairs` of metrics.json;
* LPIPS needs --vgg_weights / --lpips_weights (models.load_lpips_weights); --allow_standin_lpips reports a seeded random-feature
  distance instead and says so; with none of them the column stays empty;
* PSNR / SSIM are the published formulas of skimage (oracle/metrics_ref.py restates them) and stay unpinned against the package
  itself, which no test machine of this project has.
"""
import os
import sys

EXTENSIONS = (".png", ".jpg")


def list_images(folder):
    return sorted(n for n in os.listdir(folder) if n.lower().endswith(EXTENSIONS))


def pair_names(dir1, dir2):
    """[(name in dir1, name in dir2)] in sorted order; SystemExit on empty or unequal folders."""
    n1, n2 = list_images(dir1), list_images(dir2)
    if not n1:
        sys.exit("compare: no .png / .jpg images in " + dir1)
    if len(n1) != len(n2):
        sys.exit("compare: %d images in %s but %d in %s" % (len(n1), dir1, len(n2), dir2))
    return list(zip(n1, n2))


def decode(path, img_size=None):
    """One file -> [H,W,3] uint8 array: Image.open(p).convert('RGB') and, with img_size, the PIL-bilinear resize of load_images."""
    import numpy as np
    from PIL import Image
    img = Image.open(path).convert("RGB")
    if img_size:
        img = img.resize((img_size, img_size), Image.BILINEAR)
    return np.asarray(img, dtype=np.uint8).copy()


def decode_pairs(dir1, dir2, pairs, img_size=None):
    """[(a, b)] uint8 arrays of every pair; SystemExit where the two images of a pair differ in size."""
    out = []
    for n1, n2 in pairs:
        a, b = decode(os.path.join(dir1, n1), img_size), decode(os.path.join(dir2, n2), img_size)
        if a.shape != b.shape:
            sys.exit("compare: %s is %dx%d but %s is %dx%d (pass --img_size to resize both)"
                     % (n1, a.shape[1], a.shape[0], n2, b.shape[1], b.shape[0]))
        out.append((a, b))
    return out


def groups(arrays, batch_size):
    """index ranges of at most batch_size consecutive pairs of one image size"""
    out, start = [], 0
    for i in range(1, len(arrays) + 1):
        if i == len(arrays) or i - start == batch_size or arrays[i][0].shape != arrays[start][0].shape:
            out.append((start, i))
            start = i
    return out


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="dge_amd.compare", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--dir1", required=True, help="folder of originals")
    parser.add_argument("--dir2", required=True, help="folder of reconstructions")
    parser.add_argument("--img_size", type=int, default=None, help="resize every image to img_size x img_size (PIL bilinear)")
    parser.add_argument("--batch_size", type=int, default=8)
    parser.add_argument("--out", default="./result")
    from .infer import MetricsTable, add_lpips_args, image_metrics_rows, lpips_from_args
    add_lpips_args(parser)
    args = parser.parse_args(argv)
    if args.batch_size < 1:
        parser.error("--batch_size must be at least 1")
    pairs = pair_names(args.dir1, args.dir2)
    arrays = decode_pairs(args.dir1, args.dir2, pairs, args.img_size)
    import numpy as np
    import torch
    LP = lpips_from_args(args, "cuda")
    table = MetricsTable()
    for lo, hi in groups(arrays, args.batch_size):
        a = torch.from_numpy(np.stack([arrays[i][0] for i in range(lo, hi)])).cuda()
        b = torch.from_numpy(np.stack([arrays[i][1] for i in range(lo, hi)])).cuda()
        table.add(image_metrics_rows(a, b, LP), [p[0] for p in pairs[lo:hi]], [p[1] for p in pairs[lo:hi]])
    written = table.write(args.out, progress=print)
    for w in written:
        print(w)
    return written


if __name__ == "__main__":
    main()
