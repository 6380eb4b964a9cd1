"""Command line of the noise optimisation (dge_amd.embedding_v2 --optimize_noise): what it refuses, with which message, and its
defaults.  No GPU: parse_args builds no model."""
import pytest

from dge_amd.embedding_v2 import make_parser, noise_refusal, parse_args

BASE = ["--mtype", "2", "--optimizeE", "false"]


def test_defaults():
    a = parse_args(BASE)
    assert a.optimize_noise is False and a.noise_reg == 1e5 and a.noise_lr is None
    a = parse_args(BASE + ["--optimize_noise", "true"])
    assert a.optimize_noise is True and a.noise_reg == 1e5 and a.noise_lr is None and a.lr == 0.005
    a = parse_args(BASE + ["--optimize_noise", "true", "--noise_reg", "10", "--noise_lr", "0.1", "--independent", "true"])
    assert (a.noise_reg, a.noise_lr, a.independent) == (10.0, 0.1, True)
    with pytest.raises(SystemExit):
        make_parser().parse_args(BASE + ["--optimize_noise", "maybe"])


@pytest.mark.parametrize("argv,needle", [
    (["--mtype", "1", "--optimizeE", "false", "--optimize_noise", "true"], "is for StyleGAN2 (--mtype 2)"),
    (["--mtype", "2", "--optimizeE", "true", "--optimize_noise", "true"], "needs --optimizeE false"),
    (["--mtype", "2", "--optimizeE", "false", "--space", "z", "--optimize_noise", "true"], "not offered with --space z"),
])
def test_refusals(argv, needle):
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert "--optimize_noise true" in str(e.value) and needle in str(e.value)


def test_refuses_several_processes(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        parse_args(BASE + ["--optimize_noise", "true"])
    assert "runs in one process" in str(e.value)
    assert parse_args(BASE).optimize_noise is False          # without the flag the command line takes what it took


def test_step_refuses_with_the_same_messages():
    """LatentEmbedStep raises before it touches a model: the generator kind, the mode."""
    from dge_amd.embedding_v2 import LatentEmbedStep
    for kw, needle in ((dict(generator="sg1", mode="W"), "StyleGAN2"), (dict(generator="sg2", mode="E"), "--optimizeE false"),
                       (dict(generator="sg2", mode="Z"), "--space z")):
        with pytest.raises(ValueError, match=needle):
            LatentEmbedStep(None, None, None, optimize_noise=True, **kw)
    assert noise_refusal(True, False, False, False) is None
