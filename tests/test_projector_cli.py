"""CPU side of dge_amd.projector: the command line (defaults, strict booleans, the several-process refusal), the host schedule
against its closed-form values, the seeds of the w noise, and - on the fixture alone - the share of near-zero gradient elements
that the GPU parity test may exempt."""
import math

import numpy as np
import pytest

from tests.conftest import golden
from tests.projector_models import PROJ_ITERS


def test_parse_args_defaults(monkeypatch):
    from dge_amd.projector import parse_args
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = parse_args([])
    assert (a.steps, a.batch_size, a.lr, a.launch, a.seed, a.save_every) == (1000, 1, 0.1, "graph", 0, 100)
    assert (a.initial_noise_factor, a.noise_ramp, a.lr_rampdown, a.lr_rampup, a.noise_reg, a.w_avg_samples) == (0.05, 0.75, 0.25, 0.05, 1e5, 10000)
    assert a.mtype == 2 and a.img_size == 1024 and a.compute_dtype == "bf16" and a.checkpoint_dir_GAN is None
    assert a.deterministic is False and a.allow_standin_lpips is False and a.vgg_weights is None and a.lpips_weights is None
    b = parse_args(["--steps", "3", "--batch_size", "4", "--launch", "eager", "--allow_standin_lpips", "--checkpoint_dir_GAN", "g.pth",
                    "--img_dir", "x.pt"])
    assert (b.steps, b.batch_size, b.launch, b.allow_standin_lpips, b.checkpoint_dir_GAN, b.img_dir) == (3, 4, "eager", True, "g.pth", "x.pt")


def test_constructor_defaults_are_the_command_lines():
    import inspect
    from dge_amd.projector import ProjectorStep, parse_args, projector_schedule
    a = parse_args([])
    sig = inspect.signature(ProjectorStep.__init__).parameters
    for k in ("steps", "lr", "initial_noise_factor", "noise_ramp", "lr_rampdown", "lr_rampup", "noise_reg", "w_avg_samples", "seed"):
        assert sig[k].default == getattr(a, k), k
    sch = inspect.signature(projector_schedule).parameters
    for k in ("lr", "initial_noise_factor", "noise_ramp", "lr_rampdown", "lr_rampup"):
        assert sch[k].default == sig[k].default, k


def test_booleans_are_strict(monkeypatch):
    from dge_amd.projector import parse_args
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert parse_args(["--deterministic", "true"]).deterministic is True
    assert parse_args(["--deterministic", "false"]).deterministic is False
    for bad in ("maybe", "", "2"):
        with pytest.raises(SystemExit):
            parse_args(["--deterministic", bad])


def test_other_generators_and_several_processes_are_refused(monkeypatch):
    from dge_amd.projector import parse_args
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for mtype in ("1", "3", "4"):
        with pytest.raises(SystemExit, match="StyleGAN2"):
            parse_args(["--mtype", mtype])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        parse_args([])
    monkeypatch.setenv("WORLD_SIZE", "1")
    parse_args([])


def test_schedule_closed_form_values():
    """steps = 1000, w_std = 1, the constructor's defaults; host doubles: 1e-12."""
    from dge_amd.projector import projector_schedule
    want = {0: (0.0, 0.05), 25: (0.05, None), 500: (0.1, 0.05 / 9), 750: (None, 0.0),
            900: (0.1 * (0.5 - 0.5 * math.cos(0.4 * math.pi)), 0.0)}
    for step, (lr, ns) in want.items():
        got = projector_schedule(step, 1000, w_std=1.0)
        assert all(isinstance(v, float) for v in got)
        if lr is not None:
            assert abs(got[0] - lr) <= 1e-12, (step, got)
        if ns is not None:
            assert abs(got[1] - ns) <= 1e-12, (step, got)
    assert abs(projector_schedule(900, 1000)[0] - 0.0345492) < 1e-7
    # w_std and lr scale their outputs
    assert abs(projector_schedule(500, 1000, lr=0.2, w_std=3.0)[1] - 3.0 * 0.05 / 9) <= 1e-12
    assert abs(projector_schedule(500, 1000, lr=0.2, w_std=3.0)[0] - 0.2) <= 1e-12


def test_schedule_reproduces_the_fixture():
    from dge_amd.projector import projector_schedule
    from tests.projector_models import PROJ_SETTINGS as S
    g = golden("projector.npz")
    kw = {k: S[k] for k in ("lr", "initial_noise_factor", "noise_ramp", "lr_rampdown", "lr_rampup")}
    for it in range(PROJ_ITERS):
        lr, ns = projector_schedule(it, S["steps"], w_std=float(g["w_std"]), **kw)
        assert abs(lr - float(g[f"it{it}_lr"])) <= 1e-12
        assert np.float32(ns) == np.float32(g[f"it{it}_noise_scale"])
    assert float(g["it0_lr"]) == 0.0 and float(g["it1_lr"]) > 0.0          # the fixture holds a step that leaves w in place
    assert float(g["it1_noise_scale"]) < float(g["it0_noise_scale"])       # and the schedule moves


def test_w_noise_seeds_depend_on_image_and_iteration_only():
    from dge_amd.projector import w_noise_seed
    seen = {w_noise_seed(s, n, i) for s in (0, 1) for n in range(8) for i in range(8)}
    assert len(seen) == 128 and all(0 <= v < 1 << 64 for v in seen)
    assert w_noise_seed(3, 5, 7) == w_noise_seed(3, 5, 7)


def test_fixture_gradients_keep_the_exempt_share_inside_the_cap():
    """The GPU parity test may leave out elements whose fixture gradient is below 1e-6 of its tensor's largest (Adam's first steps
    follow the sign of the gradient) and at most 0.1 % of any tensor: the reference's own gradients stay inside that cap."""
    from tests.projector_models import EXEMPT_BELOW, EXEMPT_CAP, exempt_mask, split_maps
    g = golden("projector.npz")
    for it in range(PROJ_ITERS):
        for k, x in enumerate([g[f"it{it}_w_grad"]] + split_maps(g[f"it{it}_noise_grad"])):          # the tensors Adam steps: w and every map
            share = float(exempt_mask(x).mean())
            assert share <= EXEMPT_CAP, (it, k, share)
    assert EXEMPT_BELOW == 1e-6 and EXEMPT_CAP == 1e-3
