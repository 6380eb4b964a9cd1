"""CPU checks of the PGGAN inversion entry point (dge_amd.embedding_v2_pggan): StyleGAN1's defaults and tracker rules, strict
--optimizeE parsing, the refusals (independent with mode E, more than one process, --encoder, --truncation), --help without a GPU;
embedding_v2 itself keeps its own refusal of --mtype 3."""
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT


def test_defaults_are_stylegan1s():
    from dge_amd.embedding_v2_pggan import DEFAULTS, parse_args
    from dge_amd.embedding_v2 import DEFAULTS as V2, tracker_rules
    from dge_amd import ops
    a = parse_args([])
    assert (a.iterations, a.lr, a.beta_1, a.beta, a.norm_p, a.batch_size) == (1501, 0.005, 0.0, 1e-3, 2, 1)
    assert DEFAULTS == {k: V2[1][k] for k in DEFAULTS}
    assert a.optimizeE is True and a.independent is False and a.mtype == 3 and a.save_every == 100 and a.launch == "graph"
    assert a.encoder is None and a.truncation is None and a.deterministic is False and a.allow_standin_lpips is False
    a = parse_args(["--iterations", "30", "--lr", "0.1", "--beta", "1e-4", "--norm_p", "1", "--optimizeE", "false", "--independent", "true"])
    assert (a.iterations, a.lr, a.beta, a.norm_p, a.optimizeE, a.independent) == (30, 0.1, 1e-4, 1, False, True)
    r = tracker_rules("sg1", 1501)          # the rules PGEmbedStep takes
    assert (r["arm_rule"], r["arm_iter"], r["loss_hyst"], r["norm_hyst"], r["reset_per_group"]) == (ops.TRACK_ARM_AT, 750, 1.05, 0.0, True)


def test_optimizeE_is_parsed_strictly():
    from dge_amd.embedding_v2_pggan import parse_args
    for v, want in (("true", True), ("True", True), ("false", False), ("False", False), ("0", False), ("1", True)):
        assert parse_args(["--optimizeE", v]).optimizeE is want
    for bad in ("", "maybe", "Fals"):
        with pytest.raises(SystemExit):
            parse_args(["--optimizeE", bad])


@pytest.mark.parametrize("argv,msg", [(["--encoder", "be"], "--encoder is not offered"),
                                      (["--truncation", "0.7"], "--truncation is not offered")])
def test_flags_of_the_w_plus_loops_are_refused_with_a_message(argv, msg, capsys):
    from dge_amd.embedding_v2_pggan import parse_args
    with pytest.raises(SystemExit) as ex:
        parse_args(argv)
    assert ex.value.code != 0
    assert msg in capsys.readouterr().err


def test_independent_needs_mode_w():
    from dge_amd.embedding_v2_pggan import parse_args
    with pytest.raises(SystemExit, match="--independent true needs --optimizeE false"):
        parse_args(["--independent", "true"])
    with pytest.raises(SystemExit, match="--independent true needs --optimizeE false"):
        parse_args(["--independent", "true", "--optimizeE", "true"])


def test_more_than_one_process_is_refused(monkeypatch):
    from dge_amd.embedding_v2_pggan import parse_args
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="more than one process is not offered"):
        parse_args([])


def test_other_mtypes_are_sent_to_their_loops():
    from dge_amd.embedding_v2_pggan import parse_args
    with pytest.raises(SystemExit, match="--mtype is 3"):
        parse_args(["--mtype", "1"])


def test_step_class_refusals_need_no_gpu():
    """PGEmbedStep refuses independent with mode E and an encoder without the z head before it touches a device."""
    from dge_amd.embedding_v2_pggan import MSG_INDEPENDENT, PGEmbedStep
    from dge_amd.encoder_variants import PGBE
    from dge_amd.pggan_generator import PGGANGenerator
    G = PGGANGenerator(8, fmaps_base=64, fmaps_max=8, compute_dtype="f32")
    with pytest.raises(ValueError) as ex:
        PGEmbedStep(G, PGBE(startf=8, maxf=8, layer_count=2, pggan=True, compute_dtype="f32"), None, mode="E", independent=True)
    assert str(ex.value) == MSG_INDEPENDENT
    with pytest.raises(ValueError, match="z head"):
        PGEmbedStep(G, PGBE(startf=8, maxf=8, layer_count=2, pggan=False, compute_dtype="f32"), None, mode="W")


def test_latent_embed_step_keeps_its_generator_kinds():
    from dge_amd.embedding_v2 import LatentEmbedStep
    with pytest.raises(ValueError, match="generator must be"):
        LatentEmbedStep(None, None, None, generator="biggan")


def test_embedding_v2_still_refuses_mtype_3():
    from dge_amd.embedding_v2 import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--mtype", "3"])


def test_help_runs_without_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "dge_amd.embedding_v2_pggan", "--help"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--optimizeE" in r.stdout and "--independent" in r.stdout and "--beta" in r.stdout
