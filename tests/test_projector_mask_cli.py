"""CPU side of the masked projection: --mask_dir (parsing, pairing with the images, the count mismatch, the .pt shapes), the
float64 restatement of the masked LPIPS against oracle.lpips_ref.lpips, and - on the fixture alone - the share of near-zero
gradient elements that the GPU parity test may exempt."""
import os

import numpy as np
import pytest
import torch

from oracle import lpips_ref as LR
from tests.conftest import golden
from tests.masked_lpips_ref import mask_levels, masked_lpips, masked_value_and_grad, params64
from tests.projector_mask_models import proj_mask
from tests.projector_models import PROJ_ITERS


def test_mask_dir_flag(monkeypatch):
    from dge_amd.projector import parse_args
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert parse_args([]).mask_dir is None
    assert parse_args(["--mask_dir", "masks"]).mask_dir == "masks"
    assert parse_args(["--mask_dir", "m.pt", "--img_dir", "x.pt"]).mask_dir == "m.pt"


def test_mask_folder_pairs_with_the_images_in_sorted_name_order(tmp_path):
    from PIL import Image
    from dge_amd.projector import load_masks, mask_u8
    g = torch.Generator().manual_seed(1)
    planes = {name: torch.randint(0, 256, (16, 16), generator=g, dtype=torch.uint8) for name in ("b.png", "a.png", "c.bmp")}
    for name, p in planes.items():
        Image.fromarray(p.numpy()).save(tmp_path / name)
    (tmp_path / "notes.txt").write_text("not a mask")
    m = load_masks(str(tmp_path), 16, 3)
    assert tuple(m.shape) == (3, 1, 16, 16) and m.dtype == torch.float32
    for i, name in enumerate(("a.png", "b.png", "c.bmp")):
        assert torch.equal(m[i, 0], planes[name].float() / 255.0)          # white = 1 = fit
    assert torch.equal(mask_u8(m), torch.stack([planes[n] for n in ("a.png", "b.png", "c.bmp")]))          # mask/*.png round-trips
    # resized as the images are (PIL bilinear), still inside [0,1]
    r = load_masks(str(tmp_path), 8, 3)
    assert tuple(r.shape) == (3, 1, 8, 8) and float(r.min()) >= 0.0 and float(r.max()) <= 1.0
    want = np.asarray(Image.fromarray(planes["a.png"].numpy()).resize((8, 8), Image.BILINEAR), dtype=np.uint8)
    assert torch.equal(r[0, 0], torch.from_numpy(want.copy()).float() / 255.0)
    # an RGB file is decoded as L
    Image.fromarray(np.full((16, 16, 3), 255, dtype=np.uint8)).save(tmp_path / "d.png")
    assert torch.equal(load_masks(str(tmp_path), 16, 4)[3], torch.ones(1, 16, 16))


def test_mask_count_mismatch_exits(tmp_path):
    from PIL import Image
    from dge_amd.projector import load_masks
    Image.fromarray(np.zeros((8, 8), dtype=np.uint8)).save(tmp_path / "a.png")
    with pytest.raises(SystemExit, match="one mask per image"):
        load_masks(str(tmp_path), 8, 2)
    torch.save(torch.ones(2, 8, 8), tmp_path / "m.pt")
    with pytest.raises(SystemExit, match="one mask per image"):
        load_masks(str(tmp_path / "m.pt"), 8, 3)


def test_mask_pt_shapes(tmp_path):
    from dge_amd.projector import load_masks
    m = torch.rand(2, 8, 8, generator=torch.Generator().manual_seed(2))
    torch.save(m, tmp_path / "m3.pt")
    torch.save(m[:, None], tmp_path / "m4.pt")
    for name in ("m3.pt", "m4.pt"):
        got = load_masks(str(tmp_path / name), 8, 2)
        assert tuple(got.shape) == (2, 1, 8, 8) and torch.equal(got[:, 0], m)
    for name, bad in (("rgb.pt", torch.ones(2, 3, 8, 8)), ("flat.pt", torch.ones(8, 8)), ("size.pt", torch.ones(2, 1, 4, 4)), ("range.pt", torch.ones(2, 8, 8) * 2)):
        torch.save(bad, tmp_path / name)
        with pytest.raises(SystemExit, match="mask_dir"):
            load_masks(str(tmp_path / name), 8, 2)


def test_restatement_with_all_ones_is_lpips():
    P = params64(LR.seeded_params(0))
    g = torch.Generator().manual_seed(3)
    a = (torch.rand(2, 3, 44, 40, generator=g, dtype=torch.float64) * 2 - 1)
    b = (a * 0.7 + torch.randn(2, 3, 44, 40, generator=g, dtype=torch.float64) * 0.2).clamp(-1, 1)
    got = masked_lpips(P, a, b, torch.ones(2, 1, 44, 40, dtype=torch.float64))
    want = LR.lpips(P, a, b).reshape(2)
    assert float((got / want - 1).abs().max()) < 1e-12


def test_restatement_floor_rule_empty_levels_and_holes():
    lv = mask_levels(torch.ones(1, 1, 44, 44, dtype=torch.float64))
    assert [tuple(x.shape[2:]) for x in lv] == [(44, 44), (22, 22), (11, 11), (5, 5), (2, 2)]
    P = LR.seeded_params(0)
    g = torch.Generator().manual_seed(4)
    a, b = torch.rand(2, 3, 32, 32, generator=g) * 2 - 1, torch.rand(2, 3, 32, 32, generator=g) * 2 - 1
    m = torch.ones(2, 1, 32, 32)
    m[0] = 0                     # an empty row: 0, no gradient, nothing divides by zero
    m[1, :, :, 16:] = 0
    dist, grad = masked_value_and_grad(P, a, b, m)
    assert float(dist[0]) == 0.0 and not bool((grad[0] != 0).any()) and bool(torch.isfinite(grad).all())
    assert float(dist[1]) > 0 and not bool((grad[1, :, :, 16:] != 0).any()) and bool((grad[1, :, :, :16] != 0).any())
    a2 = a.clone()
    a2[1, :, :, 16:] = 0.25       # what lies under the mask cannot reach the result
    d2, g2 = masked_value_and_grad(P, a2, b, m)
    assert torch.equal(d2, dist) and torch.equal(g2, grad)


def test_mask_fixture_gradients_keep_the_exempt_share_inside_the_cap():
    from tests.projector_models import EXEMPT_CAP, exempt_mask, split_maps
    g = golden("projector_mask.npz")
    assert np.array_equal(g["mask"], proj_mask().numpy()) and 0.0 < float(g["mask"].mean()) < 1.0
    for it in range(PROJ_ITERS):
        for k, x in enumerate([g[f"it{it}_w_grad"]] + split_maps(g[f"it{it}_noise_grad"])):
            share = float(exempt_mask(x).mean())
            assert share <= EXEMPT_CAP, (it, k, share)
    root = os.path.dirname(os.path.abspath(__file__))
    assert os.path.getsize(os.path.join(root, "golden", "projector_mask.npz")) <= os.path.getsize(os.path.join(root, "golden", "projector.npz"))
