"""`python -m dge_amd.compare` and `python -m dge_amd.infer eval` end to end: the files they write hold the numbers of
`infer.image_metrics_rows` on the decoded bytes, to the bit (the metrics are functions of exact integer sums; PNG is lossless)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COLS = ("psnr", "ssim", "mse", "lpips", "cosine")


def _folders(tmp_path, n=4, size=(24, 20)):
    from PIL import Image
    rng = np.random.default_rng(7)
    arrs = []
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
    for i in range(n):
        a = rng.integers(0, 256, size + (3,), dtype=np.uint8)
        b = np.clip(a.astype(np.int64) + rng.integers(-30, 31, a.shape), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(tmp_path / "a" / f"im{i}.png")
        Image.fromarray(b).save(tmp_path / "b" / f"rec{i}.png")
        arrs.append((a, b))
    return arrs


def _csv(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "index,file1,file2," + ",".join(COLS)
    rows = []
    for k, ln in enumerate(lines[1:]):
        f = ln.split(",")
        assert int(f[0]) == k and len(f) == 8
        rows.append((f[1], f[2]) + tuple(None if v == "" else float(v) for v in f[3:]))
    return rows


def _check(rows, names, m, lpips=None):
    assert [r[:2] for r in rows] == names
    for i, r in enumerate(rows):
        for k, c in enumerate(COLS):
            if c == "lpips":
                assert r[2 + k] == (None if lpips is None else float(lpips[i].double())), (i, c)
            else:
                assert r[2 + k] == float(m[c][i]), (i, c, r[2 + k], float(m[c][i]))


def test_compare_writes_the_per_pair_metrics_of_the_decoded_bytes(tmp_path, capsys):
    from dge_amd import compare
    from dge_amd.infer import image_metrics_rows, load_images
    arrs = _folders(tmp_path)
    names = [(f"im{i}.png", f"rec{i}.png") for i in range(4)]
    args = ["--dir1", str(tmp_path / "a"), "--dir2", str(tmp_path / "b")]
    written = compare.main(args + ["--out", str(tmp_path / "o3"), "--batch_size", "3"])
    assert [w.split("/")[-1] for w in written] == ["metrics.csv", "metrics.json"]
    m = image_metrics_rows(torch.from_numpy(np.stack([a for a, _ in arrs])).cuda(), torch.from_numpy(np.stack([b for _, b in arrs])).cuda())
    rows = _csv(written[0])
    _check(rows, names, m)
    out = capsys.readouterr().out.splitlines()
    mean = lambda c, n: sum(r[2 + COLS.index(c)] for r in rows[:n]) / n
    assert out[0] == "img_num:1--psnr:%f--ssim:%f--mse_value:%f--lpips_value:%f--cosine_value:%f" % (
        mean("psnr", 1), mean("ssim", 1), mean("mse", 1), 0.0, mean("cosine", 1))
    assert out[3].startswith("img_num:4--psnr:%f--ssim:%f--" % (mean("psnr", 4), mean("ssim", 4)))
    js = json.load(open(written[1]))
    assert js["count"] == 4 and js["identical_pairs"] == 0 and js["lpips"] is None
    for c in ("psnr", "ssim", "mse", "cosine"):
        acc = 0.0
        for r in rows:
            acc += r[2 + COLS.index(c)]
        assert js[c] == acc / 4
    # the grouping changes nothing
    compare.main(args + ["--out", str(tmp_path / "o1"), "--batch_size", "1"])
    for f in ("metrics.csv", "metrics.json"):
        assert open(tmp_path / "o1" / f).read() == open(tmp_path / "o3" / f).read()
    # --img_size: both folders resized as load_images does
    w16 = compare.main(args + ["--out", str(tmp_path / "o16"), "--img_size", "16"])
    p1, p2 = ([str(tmp_path / d / n[k]) for n in names] for k, d in enumerate(("a", "b")))
    _check(_csv(w16[0]), names, image_metrics_rows(load_images(p1, 16), load_images(p2, 16)))
    # identical folders: infinite PSNR, counted
    wid = compare.main(["--dir1", str(tmp_path / "a"), "--dir2", str(tmp_path / "a"), "--out", str(tmp_path / "oid")])
    rid = _csv(wid[0])
    assert all(r[2] == float("inf") and r[3] == 1.0 and r[4] == 0.0 for r in rid)
    jid = json.load(open(wid[1]))
    assert jid["identical_pairs"] == 4 and jid["psnr"] == float("inf") and jid["ssim"] == 1.0


def test_compare_lpips_column_is_the_per_sample_lpips_of_the_bytes(tmp_path):
    from dge_amd import compare, ops
    from dge_amd.infer import add_lpips_args, lpips_from_args
    import argparse
    arrs = _folders(tmp_path)
    was = ops.is_deterministic()
    ops.set_deterministic(True)                      # the LPIPS head sums with f32 atomics in the default mode
    try:
        with pytest.warns(UserWarning):
            written = compare.main(["--dir1", str(tmp_path / "a"), "--dir2", str(tmp_path / "b"), "--out", str(tmp_path / "o"),
                                    "--batch_size", "4", "--allow_standin_lpips"])
            LP = lpips_from_args(add_lpips_args(argparse.ArgumentParser()).parse_args(["--allow_standin_lpips"]))
        fa, fb = (torch.from_numpy(np.stack([p[k] for p in arrs])).cuda().permute(0, 3, 1, 2).float() / 255 * 2 - 1 for k in (0, 1))
        val, _ = LP.value_and_grad(fa.contiguous(), fb.contiguous(), need_grad=False, per_sample=True)
    finally:
        ops.set_deterministic(was)
    rows = _csv(written[0])
    assert [r[5] for r in rows] == [float(v.double()) for v in val] and all(r[5] > 0 for r in rows)
    js = json.load(open(written[1]))
    assert js["lpips"] == sum(r[5] for r in rows) / 4
    with pytest.raises(RuntimeError):                 # --lpips_weights without --vgg_weights: refused as training refuses it
        compare.main(["--dir1", str(tmp_path / "a"), "--dir2", str(tmp_path / "b"), "--out", str(tmp_path / "o2"),
                      "--lpips_weights", "missing.pth"])


def test_eval_table_is_reproduced_by_compare_on_its_dump(tmp_path):
    """`infer eval --dump_dir D` (64^2 seeded StyleGAN2 + encoder from checkpoint files) and `compare` on D/real, D/rec: the same
    metrics.csv and metrics.json, byte for byte; `rec --metrics` writes the table of its own pairs."""
    from PIL import Image
    from dge_amd import compare, infer
    from dge_amd.e_align import build_models
    G, E, _ = build_models(64, 16, "bf16", device="cuda", lpips=False, seed=3, fmaps_base=2048, fmaps_max=128, enc_maxf=64)
    torch.save({"generator_smooth": G.state_dict()}, tmp_path / "g.pth")
    torch.save(E.state_dict(), tmp_path / "e.pth")
    common = ["--mtype", "2", "--img_size", "64", "--start_features", "16", "--fmaps_base", "2048", "--fmaps_max", "128",
              "--enc_maxf", "64", "--checkpoint_dir_GAN", str(tmp_path / "g.pth"), "--checkpoint_dir_E", str(tmp_path / "e.pth")]
    D = tmp_path / "dump"
    out = infer.main(["eval", "--iterations", "2", "--batch_size", "2", "--dump_dir", str(D), "--out", str(tmp_path / "oe")] + common)
    names = ["%05d.png" % i for i in range(4)]
    assert [p[len(str(D)) + 1:] for p in out[:-2]] == [f"{s}/{n}" for n in names for s in ("real", "rec")]
    assert [p.split("/")[-1] for p in out[-2:]] == ["metrics.csv", "metrics.json"]
    assert Image.open(D / "rec" / names[3]).size == (64, 64)
    rows = _csv(out[-2])
    assert [r[:2] for r in rows] == [(n, n) for n in names] and all(r[5] is None and 0 < r[4] and r[2] < 100 for r in rows)
    compare.main(["--dir1", str(D / "real"), "--dir2", str(D / "rec"), "--out", str(tmp_path / "oc"), "--batch_size", "3"])
    for f in ("metrics.csv", "metrics.json"):
        assert open(tmp_path / "oc" / f).read() == open(tmp_path / "oe" / f).read(), f
    # without --dump_dir: the table alone
    out = infer.main(["eval", "--iterations", "1", "--batch_size", "2", "--out", str(tmp_path / "oe2")] + common)
    assert [p.split("/")[-1] for p in out] == ["metrics.csv", "metrics.json"] and len(_csv(out[0])) == 2
    # rec --metrics
    src = tmp_path / "imgs"
    src.mkdir()
    rng = np.random.RandomState(0)
    for i in range(2):
        Image.fromarray(rng.randint(0, 255, (80, 72, 3), dtype=np.uint8)).save(src / f"im{i}.png")
    out = infer.main(["rec", "--img_dir", str(src), "--metrics", "--out", str(tmp_path / "or")] + common)
    assert [p.split("/")[-1] for p in out] == ["00000_realimg.png", "00000_mtv_rec.png", "00001_realimg.png", "00001_mtv_rec.png",
                                                "metrics.csv", "metrics.json"]
    rows = _csv(out[-2])
    assert [r[:2] for r in rows] == [("00000_realimg.png", "00000_mtv_rec.png"), ("00001_realimg.png", "00001_mtv_rec.png")]
    real = np.stack([np.asarray(Image.open(out[k]))[2:-2, 2:-2] for k in (0, 2)])
    rec = np.stack([np.asarray(Image.open(out[k]))[2:-2, 2:-2] for k in (1, 3)])
    _check(rows, [r[:2] for r in rows], infer.image_metrics_rows(torch.from_numpy(real).cuda(), torch.from_numpy(rec).cuda()))
