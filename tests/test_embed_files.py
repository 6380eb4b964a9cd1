"""The files the inversion loops write (dge_amd.embedding_v2.invert_v2, dge_amd.embedding_v2_pggan.invert_pg,
dge_amd.embedding_v2_biggan.invert_big, write_tracker_files): names, the text of loss_min.txt and Loss.txt, and every saved latent.  A duck-typed step stands in for the
GPU loops, so this runs on the CPU without the library.  Every expectation below is a literal recorded once from the commit before
the dump / tracker-file code was shared (this file passes there unchanged), not from the code under test.

Every saved .pt holds consecutive integers: (shape, first) below stands for arange(first, first + numel).reshape(shape)."""
import os

import pytest
import torch

B, ITERS, SAVE_EVERY, GROUP, KEEP = 3, 5, 2, 1, 2


class FakeStep:
    """step() of iteration i returns: w1 = arange(36).reshape(3,3,4) + 100*i, w_norm 2 + i (row b: + b/4), loss_msiv 0.5 + i/4 (row b:
    + b/8), infos arange(8)/2 + i + 10*k for the k-th info tensor (row b: + 100*b).  `info_img` (the "pg" form): also the window
    rows of embedding_v2's image loss, info_img[w] = the info tensor number 5 + w -> [3,8] (rows form [B,3,8])."""
    captured = False

    def __init__(self, independent, attention=True, info_img=False):
        self.independent, self.attention, self.info_img = independent, attention, info_img
        self.last = {}
        self.i = 0
        self.begun = []

    def begin_image(self, imgs1, w_init=None, labels=None):
        self.begun.append((tuple(imgs1.shape), w_init, labels))
        self.i = 0

    def step(self, imgs1):
        i, rows = self.i, self.independent
        self.i += 1
        col = torch.arange(B, dtype=torch.float32)
        r = dict(w1=torch.arange(B * 12, dtype=torch.float32).reshape(B, 3, 4) + 100 * i,
                 imgs2=torch.linspace(-1, 1, B * 3 * 8 * 8).reshape(B, 3, 8, 8),
                 w_norm=(2.0 + i + col / 4) if rows else torch.tensor(2.0 + i),
                 loss_msiv=(0.5 + i / 4 + col / 8) if rows else torch.tensor(0.5 + i / 4))
        names = ("info_mask", "info_Gcam", "info_imgs", "info_w", "info_c2") if self.attention else ("info_imgs", "info_w", "info_c2")
        for k, name in enumerate(names):
            info = torch.arange(8, dtype=torch.float32) / 2 + i + 10 * k
            r[name] = (info[None] + 100 * col[:, None]) if rows else info
        if self.info_img:
            img = torch.arange(8, dtype=torch.float32) / 2 + i + 10 * torch.arange(5, 8, dtype=torch.float32)[:, None]
            r["info_img"] = (img[None] + 100 * col[:, None, None]) if rows else img
        self.last = r
        return r

    def tracker(self):
        def one(b, shape):
            n = int(torch.Size(shape).numel())
            return dict(iteration=ITERS, dropped=0, min_loss=0.75, min_norm=1.5,
                        events=[(2, 0, 1.25 + b, 4.5), (3, 1, 1.5, 3.25 + b), (4, 0, 0.75 + b, 6.5)],
                        best_loss=torch.arange(n, dtype=torch.float32).reshape(shape) + 1000 * (b + 1),
                        best_norm=torch.arange(n, dtype=torch.float32).reshape(shape) + 5000 * (b + 1))
        return [one(b, (1, 3, 4)) for b in range(B)] if self.independent else one(0, (B, 3, 4))


def run(which, rows, tmp_path, attention=True, out=True):
    from dge_amd.embedding_v2 import invert_v2
    from dge_amd.embedding_v2_biggan import invert_big
    from dge_amd.embedding_v2_pggan import invert_pg
    out_dir = None
    if out:
        out_dir = str(tmp_path)
        for sub in ("imgs", "models"):
            os.makedirs(os.path.join(out_dir, sub))
    st = FakeStep(rows, attention, info_img=which == "pg")
    imgs1 = torch.linspace(1, -1, B * 3 * 8 * 8).reshape(B, 3, 8, 8)
    kw = dict(save_every=SAVE_EVERY, out_dir=out_dir, group=GROUP, **(dict(keep=KEEP) if rows else {}))
    if which in ("v2", "pg"):
        r = (invert_v2 if which == "v2" else invert_pg)(st, imgs1, ITERS, launch="eager", **kw)
    else:
        r = invert_big(st, imgs1, ITERS, **kw)
    assert st.i == ITERS and len(st.begun) == 1
    return st, r


def snapshot(root):
    """-> (sorted relative names, {text file: content}, {.pt file: (shape, first)}); checks the arange form of every .pt."""
    names, texts, pts = [], {}, {}
    for d, _, files in os.walk(root):
        for n in files:
            rel = os.path.relpath(os.path.join(d, n), root).replace(os.sep, "/")
            names.append(rel)
            if n.endswith(".txt"):
                with open(os.path.join(d, n)) as f:
                    texts[rel] = f.read()
            elif n.endswith(".pt"):
                t = torch.load(os.path.join(d, n))
                assert t.dtype == torch.float32
                assert torch.equal(t, torch.arange(t.numel(), dtype=torch.float32).reshape(t.shape) + t.flatten()[0]), rel
                pts[rel] = (tuple(t.shape), float(t.flatten()[0]))
    return sorted(names), texts, dict(sorted(pts.items()))


# recorded from the parent commit (see the module docstring)
EXPECT = {'v2_coupled': {'names': ['imgs/id1_ep0-norm2.00-imgLoss0.500000.jpg',
                          'imgs/id1_ep2-norm4.00-imgLoss1.000000.jpg',
                          'imgs/id1_ep4-norm6.00-imgLoss1.500000.jpg',
                          'loss_min.txt',
                          'models/id1-i0-w0-norm2.000000-imgLoss0.500000.pt',
                          'models/id1-i0-w2-norm4.000000-imgLoss1.000000.pt',
                          'models/id1-i0-w4-norm6.000000-imgLoss1.500000.pt',
                          'models/id1-i1-w0-norm2.000000-imgLoss0.500000.pt',
                          'models/id1-i1-w2-norm4.000000-imgLoss1.000000.pt',
                          'models/id1-i1-w4-norm6.000000-imgLoss1.500000.pt',
                          'models/id1-i2-w0-norm2.000000-imgLoss0.500000.pt',
                          'models/id1-i2-w2-norm4.000000-imgLoss1.000000.pt',
                          'models/id1-i2-w4-norm6.000000-imgLoss1.500000.pt',
                          'models/id1-iter3-norm-min3.250000-imgLoss1.250000.pt',
                          'models/id1-iter4-norm6.500000-imgLoss-min0.750000.pt'],
                'texts': {'loss_min.txt': 'ep1_iter2_minImg1.25000_wNorm4.500000\n'
                                          'ep1_iter3_Img1.50000_wNorm-min3.250000\n'
                                          'ep1_iter4_minImg0.75000_wNorm6.500000\n'},
                'pts': {'models/id1-i0-w0-norm2.000000-imgLoss0.500000.pt': ((1, 3, 4), 0.0),
                        'models/id1-i0-w2-norm4.000000-imgLoss1.000000.pt': ((1, 3, 4), 200.0),
                        'models/id1-i0-w4-norm6.000000-imgLoss1.500000.pt': ((1, 3, 4), 400.0),
                        'models/id1-i1-w0-norm2.000000-imgLoss0.500000.pt': ((1, 3, 4), 12.0),
                        'models/id1-i1-w2-norm4.000000-imgLoss1.000000.pt': ((1, 3, 4), 212.0),
                        'models/id1-i1-w4-norm6.000000-imgLoss1.500000.pt': ((1, 3, 4), 412.0),
                        'models/id1-i2-w0-norm2.000000-imgLoss0.500000.pt': ((1, 3, 4), 24.0),
                        'models/id1-i2-w2-norm4.000000-imgLoss1.000000.pt': ((1, 3, 4), 224.0),
                        'models/id1-i2-w4-norm6.000000-imgLoss1.500000.pt': ((1, 3, 4), 424.0),
                        'models/id1-iter3-norm-min3.250000-imgLoss1.250000.pt': ((3, 3, 4), 5000.0),
                        'models/id1-iter4-norm6.500000-imgLoss-min0.750000.pt': ((3, 3, 4), 1000.0)}},
 'v2_rows': {'names': ['imgs/id3_ep0-norm2.00-imgLoss0.500000.jpg',
                       'imgs/id3_ep2-norm4.00-imgLoss1.000000.jpg',
                       'imgs/id3_ep4-norm6.00-imgLoss1.500000.jpg',
                       'imgs/id4_ep0-norm2.25-imgLoss0.625000.jpg',
                       'imgs/id4_ep2-norm4.25-imgLoss1.125000.jpg',
                       'imgs/id4_ep4-norm6.25-imgLoss1.625000.jpg',
                       'loss_min.txt',
                       'models/id3-i0-w0-norm2.000000-imgLoss0.500000.pt',
                       'models/id3-i0-w2-norm4.000000-imgLoss1.000000.pt',
                       'models/id3-i0-w4-norm6.000000-imgLoss1.500000.pt',
                       'models/id3-iter3-norm-min3.250000-imgLoss1.250000.pt',
                       'models/id3-iter4-norm6.500000-imgLoss-min0.750000.pt',
                       'models/id4-i0-w0-norm2.250000-imgLoss0.625000.pt',
                       'models/id4-i0-w2-norm4.250000-imgLoss1.125000.pt',
                       'models/id4-i0-w4-norm6.250000-imgLoss1.625000.pt',
                       'models/id4-iter3-norm-min4.250000-imgLoss2.250000.pt',
                       'models/id4-iter4-norm6.500000-imgLoss-min1.750000.pt'],
             'texts': {'loss_min.txt': 'ep3_iter2_minImg1.25000_wNorm4.500000\n'
                                       'ep3_iter3_Img1.50000_wNorm-min3.250000\n'
                                       'ep3_iter4_minImg0.75000_wNorm6.500000\n'
                                       'ep4_iter2_minImg2.25000_wNorm4.500000\n'
                                       'ep4_iter3_Img1.50000_wNorm-min4.250000\n'
                                       'ep4_iter4_minImg1.75000_wNorm6.500000\n'},
             'pts': {'models/id3-i0-w0-norm2.000000-imgLoss0.500000.pt': ((1, 3, 4), 0.0),
                     'models/id3-i0-w2-norm4.000000-imgLoss1.000000.pt': ((1, 3, 4), 200.0),
                     'models/id3-i0-w4-norm6.000000-imgLoss1.500000.pt': ((1, 3, 4), 400.0),
                     'models/id3-iter3-norm-min3.250000-imgLoss1.250000.pt': ((1, 3, 4), 5000.0),
                     'models/id3-iter4-norm6.500000-imgLoss-min0.750000.pt': ((1, 3, 4), 1000.0),
                     'models/id4-i0-w0-norm2.250000-imgLoss0.625000.pt': ((1, 3, 4), 12.0),
                     'models/id4-i0-w2-norm4.250000-imgLoss1.125000.pt': ((1, 3, 4), 212.0),
                     'models/id4-i0-w4-norm6.250000-imgLoss1.625000.pt': ((1, 3, 4), 412.0),
                     'models/id4-iter3-norm-min4.250000-imgLoss2.250000.pt': ((1, 3, 4), 10000.0),
                     'models/id4-iter4-norm6.500000-imgLoss-min1.750000.pt': ((1, 3, 4), 2000.0)}},
 'big_coupled': {'names': ['Loss.txt',
                           'imgs/id1_ep0-norm2.00.jpg',
                           'imgs/id1_ep2-norm4.00.jpg',
                           'imgs/id1_ep4-norm6.00.jpg',
                           'loss_min.txt',
                           'models/id1-i0-w0-norm2.000000.pt',
                           'models/id1-i0-w2-norm4.000000.pt',
                           'models/id1-i0-w4-norm6.000000.pt',
                           'models/id1-i1-w0-norm2.000000.pt',
                           'models/id1-i1-w2-norm4.000000.pt',
                           'models/id1-i1-w4-norm6.000000.pt',
                           'models/id1-i2-w0-norm2.000000.pt',
                           'models/id1-i2-w2-norm4.000000.pt',
                           'models/id1-i2-w4-norm6.000000.pt',
                           'models/id1-iter3-norm-min3.250000-imgLoss1.250000.pt',
                           'models/id1-iter4-norm6.500000-imgLoss-min0.750000.pt'],
                 'texts': {'Loss.txt': 'id_1_____i_0\n'
                                       '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                       '---------ImageSpace--------\n'
                                       'loss_small_info: [[0.5, 1.0, 1.5], 2.0, 2.5, 3.0, 3.5]\n'
                                       'loss_medium_info: [[10.5, 11.0, 11.5], 12.0, 12.5, 13.0, 13.5]\n'
                                       'loss_imgs_info: [[20.5, 21.0, 21.5], 22.0, 22.5, 23.0, 23.5]\n'
                                       '---------LatentSpace--------\n'
                                       'loss_w_info: [[30.5, 31.0, 31.5], 32.0, 32.5, 33.0, 33.5]\n'
                                       'loss_c2_info: [[40.5, 41.0, 41.5], 42.0, 42.5, 43.0, 43.5]\n'
                                       'Img_loss: 0.5\n'
                                       'id_1_____i_2\n'
                                       '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                       '---------ImageSpace--------\n'
                                       'loss_small_info: [[2.5, 3.0, 3.5], 4.0, 4.5, 5.0, 5.5]\n'
                                       'loss_medium_info: [[12.5, 13.0, 13.5], 14.0, 14.5, 15.0, 15.5]\n'
                                       'loss_imgs_info: [[22.5, 23.0, 23.5], 24.0, 24.5, 25.0, 25.5]\n'
                                       '---------LatentSpace--------\n'
                                       'loss_w_info: [[32.5, 33.0, 33.5], 34.0, 34.5, 35.0, 35.5]\n'
                                       'loss_c2_info: [[42.5, 43.0, 43.5], 44.0, 44.5, 45.0, 45.5]\n'
                                       'Img_loss: 1.0\n'
                                       'id_1_____i_4\n'
                                       '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                       '---------ImageSpace--------\n'
                                       'loss_small_info: [[4.5, 5.0, 5.5], 6.0, 6.5, 7.0, 7.5]\n'
                                       'loss_medium_info: [[14.5, 15.0, 15.5], 16.0, 16.5, 17.0, 17.5]\n'
                                       'loss_imgs_info: [[24.5, 25.0, 25.5], 26.0, 26.5, 27.0, 27.5]\n'
                                       '---------LatentSpace--------\n'
                                       'loss_w_info: [[34.5, 35.0, 35.5], 36.0, 36.5, 37.0, 37.5]\n'
                                       'loss_c2_info: [[44.5, 45.0, 45.5], 46.0, 46.5, 47.0, 47.5]\n'
                                       'Img_loss: 1.5\n',
                           'loss_min.txt': 'ep1_iter2_minImg1.25000_wNorm4.500000\n'
                                           'ep1_iter3_Img1.50000_wNorm-min3.250000\n'
                                           'ep1_iter4_minImg0.75000_wNorm6.500000\n'},
                 'pts': {'models/id1-i0-w0-norm2.000000.pt': ((1, 3, 4), 0.0),
                         'models/id1-i0-w2-norm4.000000.pt': ((1, 3, 4), 200.0),
                         'models/id1-i0-w4-norm6.000000.pt': ((1, 3, 4), 400.0),
                         'models/id1-i1-w0-norm2.000000.pt': ((1, 3, 4), 12.0),
                         'models/id1-i1-w2-norm4.000000.pt': ((1, 3, 4), 212.0),
                         'models/id1-i1-w4-norm6.000000.pt': ((1, 3, 4), 412.0),
                         'models/id1-i2-w0-norm2.000000.pt': ((1, 3, 4), 24.0),
                         'models/id1-i2-w2-norm4.000000.pt': ((1, 3, 4), 224.0),
                         'models/id1-i2-w4-norm6.000000.pt': ((1, 3, 4), 424.0),
                         'models/id1-iter3-norm-min3.250000-imgLoss1.250000.pt': ((3, 3, 4), 5000.0),
                         'models/id1-iter4-norm6.500000-imgLoss-min0.750000.pt': ((3, 3, 4), 1000.0)}},
 'big_rows': {'names': ['Loss.txt',
                        'imgs/id3_ep0-norm2.00.jpg',
                        'imgs/id3_ep2-norm4.00.jpg',
                        'imgs/id3_ep4-norm6.00.jpg',
                        'imgs/id4_ep0-norm2.25.jpg',
                        'imgs/id4_ep2-norm4.25.jpg',
                        'imgs/id4_ep4-norm6.25.jpg',
                        'loss_min.txt',
                        'models/id3-i0-w0-norm2.000000.pt',
                        'models/id3-i0-w2-norm4.000000.pt',
                        'models/id3-i0-w4-norm6.000000.pt',
                        'models/id3-iter3-norm-min3.250000-imgLoss1.250000.pt',
                        'models/id3-iter4-norm6.500000-imgLoss-min0.750000.pt',
                        'models/id4-i0-w0-norm2.250000.pt',
                        'models/id4-i0-w2-norm4.250000.pt',
                        'models/id4-i0-w4-norm6.250000.pt',
                        'models/id4-iter3-norm-min4.250000-imgLoss2.250000.pt',
                        'models/id4-iter4-norm6.500000-imgLoss-min1.750000.pt'],
              'texts': {'Loss.txt': 'id_3_____i_0\n'
                                    '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                    '---------ImageSpace--------\n'
                                    'loss_small_info: [[0.5, 1.0, 1.5], 2.0, 2.5, 3.0, 3.5]\n'
                                    'loss_medium_info: [[10.5, 11.0, 11.5], 12.0, 12.5, 13.0, 13.5]\n'
                                    'loss_imgs_info: [[20.5, 21.0, 21.5], 22.0, 22.5, 23.0, 23.5]\n'
                                    '---------LatentSpace--------\n'
                                    'loss_w_info: [[30.5, 31.0, 31.5], 32.0, 32.5, 33.0, 33.5]\n'
                                    'loss_c2_info: [[40.5, 41.0, 41.5], 42.0, 42.5, 43.0, 43.5]\n'
                                    'Img_loss: 0.5\n'
                                    'id_4_____i_0\n'
                                    '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                    '---------ImageSpace--------\n'
                                    'loss_small_info: [[100.5, 101.0, 101.5], 102.0, 102.5, 103.0, 103.5]\n'
                                    'loss_medium_info: [[110.5, 111.0, 111.5], 112.0, 112.5, 113.0, 113.5]\n'
                                    'loss_imgs_info: [[120.5, 121.0, 121.5], 122.0, 122.5, 123.0, 123.5]\n'
                                    '---------LatentSpace--------\n'
                                    'loss_w_info: [[130.5, 131.0, 131.5], 132.0, 132.5, 133.0, 133.5]\n'
                                    'loss_c2_info: [[140.5, 141.0, 141.5], 142.0, 142.5, 143.0, 143.5]\n'
                                    'Img_loss: 0.625\n'
                                    'id_3_____i_2\n'
                                    '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                    '---------ImageSpace--------\n'
                                    'loss_small_info: [[2.5, 3.0, 3.5], 4.0, 4.5, 5.0, 5.5]\n'
                                    'loss_medium_info: [[12.5, 13.0, 13.5], 14.0, 14.5, 15.0, 15.5]\n'
                                    'loss_imgs_info: [[22.5, 23.0, 23.5], 24.0, 24.5, 25.0, 25.5]\n'
                                    '---------LatentSpace--------\n'
                                    'loss_w_info: [[32.5, 33.0, 33.5], 34.0, 34.5, 35.0, 35.5]\n'
                                    'loss_c2_info: [[42.5, 43.0, 43.5], 44.0, 44.5, 45.0, 45.5]\n'
                                    'Img_loss: 1.0\n'
                                    'id_4_____i_2\n'
                                    '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                    '---------ImageSpace--------\n'
                                    'loss_small_info: [[102.5, 103.0, 103.5], 104.0, 104.5, 105.0, 105.5]\n'
                                    'loss_medium_info: [[112.5, 113.0, 113.5], 114.0, 114.5, 115.0, 115.5]\n'
                                    'loss_imgs_info: [[122.5, 123.0, 123.5], 124.0, 124.5, 125.0, 125.5]\n'
                                    '---------LatentSpace--------\n'
                                    'loss_w_info: [[132.5, 133.0, 133.5], 134.0, 134.5, 135.0, 135.5]\n'
                                    'loss_c2_info: [[142.5, 143.0, 143.5], 144.0, 144.5, 145.0, 145.5]\n'
                                    'Img_loss: 1.125\n'
                                    'id_3_____i_4\n'
                                    '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                    '---------ImageSpace--------\n'
                                    'loss_small_info: [[4.5, 5.0, 5.5], 6.0, 6.5, 7.0, 7.5]\n'
                                    'loss_medium_info: [[14.5, 15.0, 15.5], 16.0, 16.5, 17.0, 17.5]\n'
                                    'loss_imgs_info: [[24.5, 25.0, 25.5], 26.0, 26.5, 27.0, 27.5]\n'
                                    '---------LatentSpace--------\n'
                                    'loss_w_info: [[34.5, 35.0, 35.5], 36.0, 36.5, 37.0, 37.5]\n'
                                    'loss_c2_info: [[44.5, 45.0, 45.5], 46.0, 46.5, 47.0, 47.5]\n'
                                    'Img_loss: 1.5\n'
                                    'id_4_____i_4\n'
                                    '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                    '---------ImageSpace--------\n'
                                    'loss_small_info: [[104.5, 105.0, 105.5], 106.0, 106.5, 107.0, 107.5]\n'
                                    'loss_medium_info: [[114.5, 115.0, 115.5], 116.0, 116.5, 117.0, 117.5]\n'
                                    'loss_imgs_info: [[124.5, 125.0, 125.5], 126.0, 126.5, 127.0, 127.5]\n'
                                    '---------LatentSpace--------\n'
                                    'loss_w_info: [[134.5, 135.0, 135.5], 136.0, 136.5, 137.0, 137.5]\n'
                                    'loss_c2_info: [[144.5, 145.0, 145.5], 146.0, 146.5, 147.0, 147.5]\n'
                                    'Img_loss: 1.625\n',
                        'loss_min.txt': 'ep3_iter2_minImg1.25000_wNorm4.500000\n'
                                        'ep3_iter3_Img1.50000_wNorm-min3.250000\n'
                                        'ep3_iter4_minImg0.75000_wNorm6.500000\n'
                                        'ep4_iter2_minImg2.25000_wNorm4.500000\n'
                                        'ep4_iter3_Img1.50000_wNorm-min4.250000\n'
                                        'ep4_iter4_minImg1.75000_wNorm6.500000\n'},
              'pts': {'models/id3-i0-w0-norm2.000000.pt': ((1, 3, 4), 0.0),
                      'models/id3-i0-w2-norm4.000000.pt': ((1, 3, 4), 200.0),
                      'models/id3-i0-w4-norm6.000000.pt': ((1, 3, 4), 400.0),
                      'models/id3-iter3-norm-min3.250000-imgLoss1.250000.pt': ((1, 3, 4), 5000.0),
                      'models/id3-iter4-norm6.500000-imgLoss-min0.750000.pt': ((1, 3, 4), 1000.0),
                      'models/id4-i0-w0-norm2.250000.pt': ((1, 3, 4), 12.0),
                      'models/id4-i0-w2-norm4.250000.pt': ((1, 3, 4), 212.0),
                      'models/id4-i0-w4-norm6.250000.pt': ((1, 3, 4), 412.0),
                      'models/id4-iter3-norm-min4.250000-imgLoss2.250000.pt': ((1, 3, 4), 10000.0),
                      'models/id4-iter4-norm6.500000-imgLoss-min1.750000.pt': ((1, 3, 4), 2000.0)}},
 'big_coupled_noatt': {'names': ['Loss.txt',
                                 'imgs/id1_ep0-norm2.00.jpg',
                                 'imgs/id1_ep2-norm4.00.jpg',
                                 'imgs/id1_ep4-norm6.00.jpg',
                                 'loss_min.txt',
                                 'models/id1-i0-w0-norm2.000000.pt',
                                 'models/id1-i0-w2-norm4.000000.pt',
                                 'models/id1-i0-w4-norm6.000000.pt',
                                 'models/id1-i1-w0-norm2.000000.pt',
                                 'models/id1-i1-w2-norm4.000000.pt',
                                 'models/id1-i1-w4-norm6.000000.pt',
                                 'models/id1-i2-w0-norm2.000000.pt',
                                 'models/id1-i2-w2-norm4.000000.pt',
                                 'models/id1-i2-w4-norm6.000000.pt',
                                 'models/id1-iter3-norm-min3.250000-imgLoss1.250000.pt',
                                 'models/id1-iter4-norm6.500000-imgLoss-min0.750000.pt'],
                       'texts': {'Loss.txt': 'id_1_____i_0\n'
                                             '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, '
                                             'loss_imgs_lpips]\n'
                                             '---------ImageSpace--------\n'
                                             'loss_imgs_info: [[0.5, 1.0, 1.5], 2.0, 2.5, 3.0, 3.5]\n'
                                             '---------LatentSpace--------\n'
                                             'loss_w_info: [[10.5, 11.0, 11.5], 12.0, 12.5, 13.0, 13.5]\n'
                                             'loss_c2_info: [[20.5, 21.0, 21.5], 22.0, 22.5, 23.0, 23.5]\n'
                                             'Img_loss: 0.5\n'
                                             'id_1_____i_2\n'
                                             '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, '
                                             'loss_imgs_lpips]\n'
                                             '---------ImageSpace--------\n'
                                             'loss_imgs_info: [[2.5, 3.0, 3.5], 4.0, 4.5, 5.0, 5.5]\n'
                                             '---------LatentSpace--------\n'
                                             'loss_w_info: [[12.5, 13.0, 13.5], 14.0, 14.5, 15.0, 15.5]\n'
                                             'loss_c2_info: [[22.5, 23.0, 23.5], 24.0, 24.5, 25.0, 25.5]\n'
                                             'Img_loss: 1.0\n'
                                             'id_1_____i_4\n'
                                             '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, '
                                             'loss_imgs_lpips]\n'
                                             '---------ImageSpace--------\n'
                                             'loss_imgs_info: [[4.5, 5.0, 5.5], 6.0, 6.5, 7.0, 7.5]\n'
                                             '---------LatentSpace--------\n'
                                             'loss_w_info: [[14.5, 15.0, 15.5], 16.0, 16.5, 17.0, 17.5]\n'
                                             'loss_c2_info: [[24.5, 25.0, 25.5], 26.0, 26.5, 27.0, 27.5]\n'
                                             'Img_loss: 1.5\n',
                                 'loss_min.txt': 'ep1_iter2_minImg1.25000_wNorm4.500000\n'
                                                 'ep1_iter3_Img1.50000_wNorm-min3.250000\n'
                                                 'ep1_iter4_minImg0.75000_wNorm6.500000\n'},
                       'pts': {'models/id1-i0-w0-norm2.000000.pt': ((1, 3, 4), 0.0),
                               'models/id1-i0-w2-norm4.000000.pt': ((1, 3, 4), 200.0),
                               'models/id1-i0-w4-norm6.000000.pt': ((1, 3, 4), 400.0),
                               'models/id1-i1-w0-norm2.000000.pt': ((1, 3, 4), 12.0),
                               'models/id1-i1-w2-norm4.000000.pt': ((1, 3, 4), 212.0),
                               'models/id1-i1-w4-norm6.000000.pt': ((1, 3, 4), 412.0),
                               'models/id1-i2-w0-norm2.000000.pt': ((1, 3, 4), 24.0),
                               'models/id1-i2-w2-norm4.000000.pt': ((1, 3, 4), 224.0),
                               'models/id1-i2-w4-norm6.000000.pt': ((1, 3, 4), 424.0),
                               'models/id1-iter3-norm-min3.250000-imgLoss1.250000.pt': ((3, 3, 4), 5000.0),
                               'models/id1-iter4-norm6.500000-imgLoss-min0.750000.pt': ((3, 3, 4), 1000.0)}},
 'big_rows_noatt': {'names': ['Loss.txt',
                              'imgs/id3_ep0-norm2.00.jpg',
                              'imgs/id3_ep2-norm4.00.jpg',
                              'imgs/id3_ep4-norm6.00.jpg',
                              'imgs/id4_ep0-norm2.25.jpg',
                              'imgs/id4_ep2-norm4.25.jpg',
                              'imgs/id4_ep4-norm6.25.jpg',
                              'loss_min.txt',
                              'models/id3-i0-w0-norm2.000000.pt',
                              'models/id3-i0-w2-norm4.000000.pt',
                              'models/id3-i0-w4-norm6.000000.pt',
                              'models/id3-iter3-norm-min3.250000-imgLoss1.250000.pt',
                              'models/id3-iter4-norm6.500000-imgLoss-min0.750000.pt',
                              'models/id4-i0-w0-norm2.250000.pt',
                              'models/id4-i0-w2-norm4.250000.pt',
                              'models/id4-i0-w4-norm6.250000.pt',
                              'models/id4-iter3-norm-min4.250000-imgLoss2.250000.pt',
                              'models/id4-iter4-norm6.500000-imgLoss-min1.750000.pt'],
                    'texts': {'Loss.txt': 'id_3_____i_0\n'
                                          '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                          '---------ImageSpace--------\n'
                                          'loss_imgs_info: [[0.5, 1.0, 1.5], 2.0, 2.5, 3.0, 3.5]\n'
                                          '---------LatentSpace--------\n'
                                          'loss_w_info: [[10.5, 11.0, 11.5], 12.0, 12.5, 13.0, 13.5]\n'
                                          'loss_c2_info: [[20.5, 21.0, 21.5], 22.0, 22.5, 23.0, 23.5]\n'
                                          'Img_loss: 0.5\n'
                                          'id_4_____i_0\n'
                                          '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                          '---------ImageSpace--------\n'
                                          'loss_imgs_info: [[100.5, 101.0, 101.5], 102.0, 102.5, 103.0, 103.5]\n'
                                          '---------LatentSpace--------\n'
                                          'loss_w_info: [[110.5, 111.0, 111.5], 112.0, 112.5, 113.0, 113.5]\n'
                                          'loss_c2_info: [[120.5, 121.0, 121.5], 122.0, 122.5, 123.0, 123.5]\n'
                                          'Img_loss: 0.625\n'
                                          'id_3_____i_2\n'
                                          '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                          '---------ImageSpace--------\n'
                                          'loss_imgs_info: [[2.5, 3.0, 3.5], 4.0, 4.5, 5.0, 5.5]\n'
                                          '---------LatentSpace--------\n'
                                          'loss_w_info: [[12.5, 13.0, 13.5], 14.0, 14.5, 15.0, 15.5]\n'
                                          'loss_c2_info: [[22.5, 23.0, 23.5], 24.0, 24.5, 25.0, 25.5]\n'
                                          'Img_loss: 1.0\n'
                                          'id_4_____i_2\n'
                                          '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                          '---------ImageSpace--------\n'
                                          'loss_imgs_info: [[102.5, 103.0, 103.5], 104.0, 104.5, 105.0, 105.5]\n'
                                          '---------LatentSpace--------\n'
                                          'loss_w_info: [[112.5, 113.0, 113.5], 114.0, 114.5, 115.0, 115.5]\n'
                                          'loss_c2_info: [[122.5, 123.0, 123.5], 124.0, 124.5, 125.0, 125.5]\n'
                                          'Img_loss: 1.125\n'
                                          'id_3_____i_4\n'
                                          '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                          '---------ImageSpace--------\n'
                                          'loss_imgs_info: [[4.5, 5.0, 5.5], 6.0, 6.5, 7.0, 7.5]\n'
                                          '---------LatentSpace--------\n'
                                          'loss_w_info: [[14.5, 15.0, 15.5], 16.0, 16.5, 17.0, 17.5]\n'
                                          'loss_c2_info: [[24.5, 25.0, 25.5], 26.0, 26.5, 27.0, 27.5]\n'
                                          'Img_loss: 1.5\n'
                                          'id_4_____i_4\n'
                                          '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
                                          '---------ImageSpace--------\n'
                                          'loss_imgs_info: [[104.5, 105.0, 105.5], 106.0, 106.5, 107.0, 107.5]\n'
                                          '---------LatentSpace--------\n'
                                          'loss_w_info: [[114.5, 115.0, 115.5], 116.0, 116.5, 117.0, 117.5]\n'
                                          'loss_c2_info: [[124.5, 125.0, 125.5], 126.0, 126.5, 127.0, 127.5]\n'
                                          'Img_loss: 1.625\n',
                              'loss_min.txt': 'ep3_iter2_minImg1.25000_wNorm4.500000\n'
                                              'ep3_iter3_Img1.50000_wNorm-min3.250000\n'
                                              'ep3_iter4_minImg0.75000_wNorm6.500000\n'
                                              'ep4_iter2_minImg2.25000_wNorm4.500000\n'
                                              'ep4_iter3_Img1.50000_wNorm-min4.250000\n'
                                              'ep4_iter4_minImg1.75000_wNorm6.500000\n'},
                    'pts': {'models/id3-i0-w0-norm2.000000.pt': ((1, 3, 4), 0.0),
                            'models/id3-i0-w2-norm4.000000.pt': ((1, 3, 4), 200.0),
                            'models/id3-i0-w4-norm6.000000.pt': ((1, 3, 4), 400.0),
                            'models/id3-iter3-norm-min3.250000-imgLoss1.250000.pt': ((1, 3, 4), 5000.0),
                            'models/id3-iter4-norm6.500000-imgLoss-min0.750000.pt': ((1, 3, 4), 1000.0),
                            'models/id4-i0-w0-norm2.250000.pt': ((1, 3, 4), 12.0),
                            'models/id4-i0-w2-norm4.250000.pt': ((1, 3, 4), 212.0),
                            'models/id4-i0-w4-norm6.250000.pt': ((1, 3, 4), 412.0),
                            'models/id4-iter3-norm-min4.250000-imgLoss2.250000.pt': ((1, 3, 4), 10000.0),
                            'models/id4-iter4-norm6.500000-imgLoss-min1.750000.pt': ((1, 3, 4), 2000.0)}}}

# The "pg" forms (embedding_v2_pggan.invert_pg), recorded from the commit before the three per-group loops were shared with only this
# file changed: the names, loss_min.txt and the saved latents are those of the "v2" forms, plus a Loss.txt whose image-space lines
# are the window rows of `info_img` (small = row 2, medium = row 1, imgs = row 0).
_HEAD = '[loss_imgs_mse[img,img_mean,img_std], loss_imgs_kl, loss_imgs_cosine, loss_imgs_ssim, loss_imgs_lpips]\n'
_PG_LOSS_TXT = {
    'pg_coupled': 'id_1_____i_0\n' + _HEAD +
                  '---------ImageSpace--------\n'
                  'loss_small_info: [[70.5, 71.0, 71.5], 72.0, 72.5, 73.0, 73.5]\n'
                  'loss_medium_info: [[60.5, 61.0, 61.5], 62.0, 62.5, 63.0, 63.5]\n'
                  'loss_imgs_info: [[50.5, 51.0, 51.5], 52.0, 52.5, 53.0, 53.5]\n'
                  '---------LatentSpace--------\n'
                  'loss_w_info: [[30.5, 31.0, 31.5], 32.0, 32.5, 33.0, 33.5]\n'
                  'loss_c2_info: [[40.5, 41.0, 41.5], 42.0, 42.5, 43.0, 43.5]\n'
                  'Img_loss: 0.5\n'
                  'id_1_____i_2\n' + _HEAD +
                  '---------ImageSpace--------\n'
                  'loss_small_info: [[72.5, 73.0, 73.5], 74.0, 74.5, 75.0, 75.5]\n'
                  'loss_medium_info: [[62.5, 63.0, 63.5], 64.0, 64.5, 65.0, 65.5]\n'
                  'loss_imgs_info: [[52.5, 53.0, 53.5], 54.0, 54.5, 55.0, 55.5]\n'
                  '---------LatentSpace--------\n'
                  'loss_w_info: [[32.5, 33.0, 33.5], 34.0, 34.5, 35.0, 35.5]\n'
                  'loss_c2_info: [[42.5, 43.0, 43.5], 44.0, 44.5, 45.0, 45.5]\n'
                  'Img_loss: 1.0\n'
                  'id_1_____i_4\n' + _HEAD +
                  '---------ImageSpace--------\n'
                  'loss_small_info: [[74.5, 75.0, 75.5], 76.0, 76.5, 77.0, 77.5]\n'
                  'loss_medium_info: [[64.5, 65.0, 65.5], 66.0, 66.5, 67.0, 67.5]\n'
                  'loss_imgs_info: [[54.5, 55.0, 55.5], 56.0, 56.5, 57.0, 57.5]\n'
                  '---------LatentSpace--------\n'
                  'loss_w_info: [[34.5, 35.0, 35.5], 36.0, 36.5, 37.0, 37.5]\n'
                  'loss_c2_info: [[44.5, 45.0, 45.5], 46.0, 46.5, 47.0, 47.5]\n'
                  'Img_loss: 1.5\n',
    'pg_rows': 'id_3_____i_0\n' + _HEAD +
               '---------ImageSpace--------\n'
               'loss_small_info: [[70.5, 71.0, 71.5], 72.0, 72.5, 73.0, 73.5]\n'
               'loss_medium_info: [[60.5, 61.0, 61.5], 62.0, 62.5, 63.0, 63.5]\n'
               'loss_imgs_info: [[50.5, 51.0, 51.5], 52.0, 52.5, 53.0, 53.5]\n'
               '---------LatentSpace--------\n'
               'loss_w_info: [[30.5, 31.0, 31.5], 32.0, 32.5, 33.0, 33.5]\n'
               'loss_c2_info: [[40.5, 41.0, 41.5], 42.0, 42.5, 43.0, 43.5]\n'
               'Img_loss: 0.5\n'
               'id_4_____i_0\n' + _HEAD +
               '---------ImageSpace--------\n'
               'loss_small_info: [[170.5, 171.0, 171.5], 172.0, 172.5, 173.0, 173.5]\n'
               'loss_medium_info: [[160.5, 161.0, 161.5], 162.0, 162.5, 163.0, 163.5]\n'
               'loss_imgs_info: [[150.5, 151.0, 151.5], 152.0, 152.5, 153.0, 153.5]\n'
               '---------LatentSpace--------\n'
               'loss_w_info: [[130.5, 131.0, 131.5], 132.0, 132.5, 133.0, 133.5]\n'
               'loss_c2_info: [[140.5, 141.0, 141.5], 142.0, 142.5, 143.0, 143.5]\n'
               'Img_loss: 0.625\n'
               'id_3_____i_2\n' + _HEAD +
               '---------ImageSpace--------\n'
               'loss_small_info: [[72.5, 73.0, 73.5], 74.0, 74.5, 75.0, 75.5]\n'
               'loss_medium_info: [[62.5, 63.0, 63.5], 64.0, 64.5, 65.0, 65.5]\n'
               'loss_imgs_info: [[52.5, 53.0, 53.5], 54.0, 54.5, 55.0, 55.5]\n'
               '---------LatentSpace--------\n'
               'loss_w_info: [[32.5, 33.0, 33.5], 34.0, 34.5, 35.0, 35.5]\n'
               'loss_c2_info: [[42.5, 43.0, 43.5], 44.0, 44.5, 45.0, 45.5]\n'
               'Img_loss: 1.0\n'
               'id_4_____i_2\n' + _HEAD +
               '---------ImageSpace--------\n'
               'loss_small_info: [[172.5, 173.0, 173.5], 174.0, 174.5, 175.0, 175.5]\n'
               'loss_medium_info: [[162.5, 163.0, 163.5], 164.0, 164.5, 165.0, 165.5]\n'
               'loss_imgs_info: [[152.5, 153.0, 153.5], 154.0, 154.5, 155.0, 155.5]\n'
               '---------LatentSpace--------\n'
               'loss_w_info: [[132.5, 133.0, 133.5], 134.0, 134.5, 135.0, 135.5]\n'
               'loss_c2_info: [[142.5, 143.0, 143.5], 144.0, 144.5, 145.0, 145.5]\n'
               'Img_loss: 1.125\n'
               'id_3_____i_4\n' + _HEAD +
               '---------ImageSpace--------\n'
               'loss_small_info: [[74.5, 75.0, 75.5], 76.0, 76.5, 77.0, 77.5]\n'
               'loss_medium_info: [[64.5, 65.0, 65.5], 66.0, 66.5, 67.0, 67.5]\n'
               'loss_imgs_info: [[54.5, 55.0, 55.5], 56.0, 56.5, 57.0, 57.5]\n'
               '---------LatentSpace--------\n'
               'loss_w_info: [[34.5, 35.0, 35.5], 36.0, 36.5, 37.0, 37.5]\n'
               'loss_c2_info: [[44.5, 45.0, 45.5], 46.0, 46.5, 47.0, 47.5]\n'
               'Img_loss: 1.5\n'
               'id_4_____i_4\n' + _HEAD +
               '---------ImageSpace--------\n'
               'loss_small_info: [[174.5, 175.0, 175.5], 176.0, 176.5, 177.0, 177.5]\n'
               'loss_medium_info: [[164.5, 165.0, 165.5], 166.0, 166.5, 167.0, 167.5]\n'
               'loss_imgs_info: [[154.5, 155.0, 155.5], 156.0, 156.5, 157.0, 157.5]\n'
               '---------LatentSpace--------\n'
               'loss_w_info: [[134.5, 135.0, 135.5], 136.0, 136.5, 137.0, 137.5]\n'
               'loss_c2_info: [[144.5, 145.0, 145.5], 146.0, 146.5, 147.0, 147.5]\n'
               'Img_loss: 1.625\n'}
for _form, _txt in _PG_LOSS_TXT.items():
    _v2 = EXPECT["v2" + _form[2:]]
    EXPECT[_form] = dict(names=["Loss.txt"] + _v2["names"], texts=dict(_v2["texts"], **{"Loss.txt": _txt}), pts=_v2["pts"])


@pytest.mark.parametrize("form", ["v2_coupled", "v2_rows", "big_coupled", "big_rows", "big_coupled_noatt", "big_rows_noatt", "pg_coupled",
                                  "pg_rows"])
def test_files_of_an_inversion(form, tmp_path):
    which, kind = form.split("_", 1)
    st, r = run(which, kind.startswith("rows"), tmp_path, attention=not kind.endswith("noatt"))
    names, texts, pts = snapshot(str(tmp_path))
    want = EXPECT[form]
    assert names == want["names"]
    assert texts == want["texts"]
    assert pts == want["pts"]
    assert sorted(pts) == [n for n in names if n.endswith(".pt")]
    assert isinstance(r["tracker"], list if st.independent else dict) and "tracker" not in st.last
    assert torch.equal(r["w1"], st.last["w1"])


@pytest.mark.parametrize("which", ["v2", "big", "pg"])
@pytest.mark.parametrize("rows", [False, True])
def test_without_out_dir_nothing_is_written(which, rows, tmp_path):
    st, r = run(which, rows, tmp_path, out=False)
    assert os.listdir(str(tmp_path)) == []
    tr = r["tracker"]
    if rows:
        assert isinstance(tr, list) and len(tr) == B and [t["events"][0][2] for t in tr] == [1.25, 2.25, 3.25]
    else:
        assert isinstance(tr, dict) and tr["events"] == st.tracker()["events"]
    assert torch.equal(r["w1"], st.last["w1"]) and "tracker" not in st.last


def test_tracker_files_with_norm_events_only(tmp_path):
    """Without a best-loss event the norm file's imgLoss is 0.000000 and no best-loss file appears."""
    from dge_amd.embedding_v2 import EVENT_NORM, write_tracker_files
    models = tmp_path / "models"
    models.mkdir()
    tr = dict(events=[(7, EVENT_NORM, 0.5, 3.0), (9, EVENT_NORM, 0.625, 2.5)], best_loss=torch.zeros(1, 2), best_norm=torch.arange(2.0).reshape(1, 2))
    write_tracker_files(tr, 4, str(models), str(tmp_path))
    names, texts, pts = snapshot(str(tmp_path))
    assert names == ["loss_min.txt", "models/id4-iter9-norm-min2.500000-imgLoss0.000000.pt"]
    assert texts == {"loss_min.txt": "ep4_iter7_Img0.50000_wNorm-min3.000000\nep4_iter9_Img0.62500_wNorm-min2.500000\n"}
    assert pts == {"models/id4-iter9-norm-min2.500000-imgLoss0.000000.pt": ((1, 2), 0.0)}
