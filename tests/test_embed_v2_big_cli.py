"""CPU checks of the BigGAN-deep inversion entry point (dge_amd.embedding_v2_biggan): the defaults of the reference's script
(embedding_v2_BigGAN.py:234-248, :37,43), strict --optimizeE parsing, the refused --beta / --norm_p, --help without a GPU."""
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT


def test_defaults_are_the_scripts():
    from dge_amd.embedding_v2_biggan import BIGGAN_DEEP256, parse_args
    from dge_amd.embedding_v2 import tracker_rules
    from dge_amd import ops
    a = parse_args([])
    assert (a.iterations, a.lr, a.beta_1, a.batch_size, a.img_size, a.z_dim, a.start_features, a.label, a.truncation) == \
        (1501, 0.0003, 0.0, 1, 256, 128, 64, 30, 0.4)
    assert a.optimizeE is True and a.attention is True and a.mtype == 4 and a.save_every == 100
    assert a.beta is None and a.norm_p is None and a.deterministic is False and a.allow_standin_lpips is False
    a = parse_args(["--iterations", "30", "--lr", "0.1", "--label", "207", "--attention", "false", "--truncation", "0.5"])
    assert (a.iterations, a.lr, a.label, a.attention, a.truncation) == (30, 0.1, 207, False, 0.5)
    with pytest.raises(SystemExit):
        parse_args(["--mtype", "2"])
    r = tracker_rules("sg1", a.iterations)          # the rules BigEmbedStep takes
    assert (r["arm_rule"], r["arm_iter"], r["loss_hyst"], r["norm_hyst"], r["reset_per_group"]) == (ops.TRACK_ARM_AT, 15, 1.05, 0.0, True)
    assert BIGGAN_DEEP256["output_dim"] == 256 and len(BIGGAN_DEEP256["layers"]) == 12


def test_optimizeE_is_parsed_strictly():
    from dge_amd.embedding_v2_biggan import parse_args
    for v, want in (("true", True), ("True", True), ("false", False), ("False", False), ("0", False), ("1", True)):
        assert parse_args(["--optimizeE", v]).optimizeE is want
    for bad in ("", "maybe", "Fals"):
        with pytest.raises(SystemExit):
            parse_args(["--optimizeE", bad])


@pytest.mark.parametrize("flag,value", [("--beta", "1e-6"), ("--norm_p", "2")])
def test_the_norm_term_is_rejected(flag, value, capsys):
    from dge_amd.embedding_v2_biggan import parse_args
    with pytest.raises(SystemExit) as ex:
        parse_args([flag, value])
    assert ex.value.code != 0
    assert "not offered" in capsys.readouterr().err


def test_embedding_v2_still_refuses_mtype_4():
    from dge_amd.embedding_v2 import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--mtype", "4"])


def test_help_runs_without_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "dge_amd.embedding_v2_biggan", "--help"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--optimizeE" in r.stdout and "--attention" in r.stdout and "--label" in r.stdout
