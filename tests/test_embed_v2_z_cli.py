"""Command line and file side of the Z-space inversion (dge_amd.embedding_v2 --optimizeE false --space z) and the C-ABI surface of
the chip-wide mapping adjoint; runs on the CPU without the library (a duck-typed step stands in for the GPU loop, as in
test_embed_files.py)."""
import os
import re

import pytest
import torch

from tests.conftest import ROOT

B = 2


def test_space_z_parses_with_the_per_mtype_defaults():
    from dge_amd.embedding_v2 import DEFAULTS, parse_args
    a = parse_args(["--optimizeE", "false", "--space", "z", "--mtype", "2"])
    assert a.space == "z" and a.optimizeE is False and a.truncation == 0.7 and a.iterations == DEFAULTS[2]["iterations"]
    a = parse_args(["--optimizeE", "false", "--space", "z", "--independent", "true", "--batch_size", "3"])
    assert a.space == "z" and a.mtype == 1 and a.independent and a.beta == DEFAULTS[1]["beta"]


def test_default_parse_is_unchanged():
    from dge_amd.embedding_v2 import DEFAULTS, parse_args
    a = parse_args([])
    assert a.space == "w" and a.optimizeE is True and a.mtype == 1 and a.independent is False
    assert {k: getattr(a, k) for k in DEFAULTS[1]} == DEFAULTS[1]
    b = vars(parse_args(["--optimizeE", "false", "--mtype", "2"]))
    assert b.pop("space") == "w" and b["truncation"] == 0.7 and b["launch"] == "graph" and b["batch_size"] == 1


@pytest.mark.parametrize("argv,msg", [
    (["--space", "z"], "--space z needs --optimizeE false"),
    (["--space", "z", "--optimizeE", "true"], "--space z needs --optimizeE false"),
    (["--space", "z", "--optimizeE", "false", "--mtype", "3"], "--space z is for --mtype 1"),
    (["--space", "z", "--optimizeE", "false", "--mtype", "4"], "--space z is for --mtype 1"),
])
def test_space_z_refusals(argv, msg):
    from dge_amd.embedding_v2 import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert msg in str(e.value)


def test_space_z_refuses_more_than_one_process(monkeypatch):
    from dge_amd.embedding_v2 import parse_args
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        parse_args(["--space", "z", "--optimizeE", "false"])
    assert "one process" in str(e.value)
    assert parse_args(["--optimizeE", "false"]).space == "w"          # W space is not affected


def test_step_refuses_z_mode_where_it_has_no_meaning():
    from dge_amd.embedding_v2 import LatentEmbedStep
    with pytest.raises(ValueError, match="PGGAN"):
        LatentEmbedStep(None, None, None, mode="Z", generator="pg")
    with pytest.raises(ValueError, match="Gm"):
        LatentEmbedStep(None, None, None, mode="Z", generator="sg1")
    with pytest.raises(ValueError, match="mode must be"):
        LatentEmbedStep(None, None, None, mode="Y", generator="sg2")


def test_header_and_bindings_carry_the_wide_adjoint():
    from dge_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dge_hip.h")).read()
    for name in ("dge_mapping_bwd_wide", "dge_mapping_bwd_wide_work_bytes"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["dge_mapping_bwd_wide"]) == len(_lib.SIGNATURES["dge_mapping_bwd"]) + 2          # + work, work_bytes
    assert "dge_mapping_bwd_wide" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


class FakeZStep:
    """A mode-"Z" step: the latent of the result is z [B, 512]."""
    captured = False
    mode = "Z"

    def __init__(self, independent):
        self.independent, self.last, self.i = independent, {}, 0

    def begin_image(self, imgs1, w_init=None):
        self.i = 0

    def step(self, imgs1):
        i, rows = self.i, self.independent
        self.i += 1
        col = torch.arange(B, dtype=torch.float32)
        self.last = dict(w1=torch.arange(B * 512, dtype=torch.float32).reshape(B, 512) + i, imgs2=torch.zeros(B, 3, 8, 8),
                         w_norm=(2.0 + i + col) if rows else torch.tensor(2.0 + i), loss_msiv=(0.5 + col) if rows else torch.tensor(0.5))
        return self.last

    def tracker(self):
        one = lambda shape: dict(iteration=3, dropped=0, min_loss=0.5, min_norm=1.5, events=[(2, 0, 0.5, 4.0)],
                                 best_loss=torch.zeros(shape), best_norm=torch.zeros(shape))
        return [one((1, 512)) for _ in range(B)] if self.independent else one((B, 512))


@pytest.mark.parametrize("rows", [False, True])
def test_dump_and_finish_write_the_z_mode_names(rows, tmp_path):
    from dge_amd.embedding_v2 import invert_folder, invert_v2
    out = str(tmp_path)
    for sub in ("imgs", "models", "summaries"):
        os.makedirs(os.path.join(out, sub))
    st = FakeZStep(rows)
    imgs = torch.zeros(2 * B, 3, 8, 8)
    invert_folder(lambda imgs1, **kw: invert_v2(st, imgs1, 3, launch="eager", save_every=2, out_dir=out, **kw), imgs, B, rows, out,
                  all_name="z_all_%d.pt")
    names = sorted(os.listdir(os.path.join(out, "models")))
    latents = [n for n in names if re.fullmatch(r"id\d+-i\d+-z\d+-norm[\d.]+-imgLoss[\d.]+\.pt", n)]
    assert not any(re.search(r"-w\d+-", n) or n.startswith("w_all") for n in names), names
    if rows:          # numbered by image: 4 images x iterations 0 and 2, one row each
        assert len(latents) == 8 and "id3-i0-z2-norm5.000000-imgLoss1.500000.pt" in latents, latents
        assert "z_all_3.pt" in names and tuple(torch.load(os.path.join(out, "models", "z_all_3.pt")).shape) == (4, 512)
    else:             # numbered by group: 2 groups x iterations 0 and 2 x the rows of the file set
        assert len(latents) == 8 and "id1-i1-z2-norm4.000000-imgLoss0.500000.pt" in latents, latents
        assert "z_all_1.pt" in names and tuple(torch.load(os.path.join(out, "models", "z_all_1.pt")).shape) == (2, 512)
    z = torch.load(os.path.join(out, "models", latents[0]))
    assert tuple(z.shape) == (1, 512)
    assert any(n.endswith("imgLoss-min0.500000.pt") for n in names)          # the tracker's files keep their names
