"""CPU checks of the v2 inversion entry point (dge_amd.embedding_v2): per-`--mtype` defaults of the reference's scripts
(embedding_v2_styleGAN1.py:195-209, embedding_v2_styleGAN2.py:214-232), strict --optimizeE parsing, --help without a GPU."""
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT


def test_per_mtype_defaults():
    from dge_amd.embedding_v2 import parse_args, tracker_rules
    from dge_amd import ops
    a1 = parse_args(["--mtype", "1"])
    assert (a1.iterations, a1.lr, a1.beta_1, a1.beta, a1.norm_p, a1.truncation) == (1501, 0.005, 0.0, 1e-3, 2, None)
    a2 = parse_args(["--mtype", "2"])
    assert (a2.iterations, a2.lr, a2.beta_1, a2.beta, a2.norm_p, a2.truncation) == (2001, 0.005, 0.0, 3e-4, 2, 0.7)
    assert parse_args([]).mtype == 1                                          # the reference's default
    a = parse_args(["--mtype", "2", "--iterations", "30", "--beta", "0.01", "--norm_p", "3", "--truncation", "1", "--lr", "0.1"])
    assert (a.iterations, a.beta, a.norm_p, a.truncation, a.lr) == (30, 0.01, 3, 1.0, 0.1)
    r1 = tracker_rules("sg1", 1501)
    assert (r1["arm_rule"], r1["arm_iter"], r1["loss_hyst"], r1["norm_hyst"], r1["init"], r1["reset_per_group"]) == \
        (ops.TRACK_ARM_AT, 750, 1.05, 0.0, (0.0, 0.0), True)
    r2 = tracker_rules("sg2", 2001)
    assert (r2["arm_rule"], r2["arm_iter"], r2["loss_hyst"], r2["norm_hyst"], r2["init"], r2["reset_per_group"]) == \
        (ops.TRACK_ARM_AFTER, 1000, 1.03, 1.05, (100.0, 1000.0), False)
    with pytest.raises(SystemExit):
        parse_args(["--mtype", "4"])


def test_optimizeE_is_parsed_strictly():
    from dge_amd.embedding_v2 import parse_args
    assert parse_args([]).optimizeE is True
    for v, want in (("true", True), ("True", True), ("false", False), ("False", False), ("0", False), ("1", True)):
        assert parse_args(["--optimizeE", v]).optimizeE is want
    for bad in ("", "maybe", "Fals"):
        with pytest.raises(SystemExit):
            parse_args(["--optimizeE", bad])


def test_help_runs_without_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "dge_amd.embedding_v2", "--help"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--optimizeE" in r.stdout and "--truncation" in r.stdout
