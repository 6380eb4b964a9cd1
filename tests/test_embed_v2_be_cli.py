"""`embedding_v2 --encoder`: the command line accepts E_Blur (default) or E.BE, and nothing else."""
import pytest


def test_encoder_flag_parses_be_and_refuses_others(capsys):
    from dge_amd.embedding_v2 import ENCODERS, make_parser, parse_args
    assert ENCODERS == ("blur", "be")
    assert make_parser().parse_args([]).encoder == "blur"
    for mtype in ("1", "2"):
        args = parse_args(["--mtype", mtype, "--encoder", "be", "--optimizeE", "false"])
        assert args.encoder == "be" and args.optimizeE is False
    with pytest.raises(SystemExit):
        make_parser().parse_args(["--encoder", "x"])
    assert "--encoder" in capsys.readouterr().err


def test_build_models_v2_refuses_an_unknown_encoder():
    from dge_amd.embedding_v2 import build_models_v2
    with pytest.raises(ValueError, match="encoder"):
        build_models_v2(2, 64, device="cpu", encoder="x")
