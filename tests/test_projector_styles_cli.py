"""CPU side of the projector's StyleSpace stage: the command line (`--s_steps 0` by default, refusals with their messages), the
stage's defaults and schedule, the file names, and - on the fixture alone - the share of near-zero gradient elements that the GPU
parity test may exempt."""
import numpy as np
import pytest
import torch

from tests.conftest import golden
from tests.projector_models import EXEMPT_BELOW, EXEMPT_CAP, PROJ_B, PROJ_ITERS, exempt_mask, split_maps
from tests.s2_style_models import S64_CHANNELS, STYLE_SETTINGS, split_blocks


def test_parse_args_defaults_and_refusals(monkeypatch):
    from dge_amd.projector import parse_args
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = parse_args([])
    assert a.s_steps == 0 and a.s_lr == 0.01
    b = parse_args(["--s_steps", "50", "--s_lr", "0.02"])
    assert (b.s_steps, b.s_lr) == (50, 0.02)
    with pytest.raises(SystemExit, match="--s_steps must be 0"):
        parse_args(["--s_steps", "-1"])
    with pytest.raises(SystemExit, match="--s_lr must be positive"):
        parse_args(["--s_steps", "5", "--s_lr", "0"])
    parse_args(["--s_lr", "0"])          # (without a stage the rate is not read)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        parse_args(["--s_steps", "5"])


def test_stage_defaults_and_refusals(monkeypatch):
    import inspect
    from dge_amd.projector import StyleProjectorStep, parse_args
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    sig = inspect.signature(StyleProjectorStep.__init__).parameters
    a = parse_args([])
    assert sig["lr"].default == a.s_lr == 0.01
    for k in ("lr_rampdown", "lr_rampup", "noise_reg"):
        assert sig[k].default == getattr(a, k), k

    class G(torch.nn.Module):
        pass
    g = G().eval()
    with pytest.raises(ValueError, match="steps must be positive"):
        StyleProjectorStep(g, None, steps=0)
    with pytest.raises(ValueError, match="eval mode"):
        StyleProjectorStep(G().train(), None)
    st = StyleProjectorStep(g, None, steps=4)
    with pytest.raises(RuntimeError, match="begin_image"):
        st.step(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no captured iteration"):
        st.set_image(torch.zeros(1, 3, 8, 8))
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)          # (the constructor looks at the process group)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda: 2)
    with pytest.raises(ValueError, match="one process"):
        StyleProjectorStep(g, None)


def test_stage_schedule_is_the_projectors_ramp_without_noise():
    from dge_amd.projector import StyleProjectorStep, projector_schedule

    class G(torch.nn.Module):
        pass
    S = STYLE_SETTINGS
    st = StyleProjectorStep(G().eval(), None, **S)
    g = golden("projector_styles.npz")
    for it in range(PROJ_ITERS):
        assert st.schedule(it) == projector_schedule(it, S["steps"], S["lr"], lr_rampdown=S["lr_rampdown"], lr_rampup=S["lr_rampup"])[0]
        assert abs(st.schedule(it) - float(g[f"it{it}_lr"])) <= 1e-12
    assert float(g["it0_lr"]) == 0.0 and float(g["it1_lr"]) == S["lr"]          # the fixture holds a step that leaves the codes in place


def test_file_names_of_the_codes(tmp_path):
    import os
    from dge_amd.stylegan2_generator import SynthesisModule
    from dge_amd.style_codes import StyleCodes, save_style_rows
    from tests.s2_noise_models import S2N_KW
    c = StyleCodes(SynthesisModule(64, compute_dtype="f32", **S2N_KW), 2, "cpu")
    save_style_rows(c, range(2), [4, 11], str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["id11-s.pt", "id4-s.pt"]
    rows = torch.load(tmp_path / "id4-s.pt")
    assert isinstance(rows, list) and [tuple(r.shape) for r in rows] == [(1, C) for C in S64_CHANNELS]


def test_fixture_gradients_keep_the_exempt_share_inside_the_cap():
    """The GPU parity test may leave out elements whose fixture gradient is below 1e-6 of its tensor's largest, at most 0.1 % of any
    tensor: the reference's own gradients of the style blocks hold none at all, and those of the maps stay inside the cap."""
    g = golden("projector_styles.npz")
    for it in range(PROJ_ITERS):
        for k, x in enumerate(split_blocks(g[f"it{it}_style_grad"], PROJ_B)):
            assert int(exempt_mask(x).sum()) == 0, (it, k)
        for k, x in enumerate(split_maps(g[f"it{it}_noise_grad"])):
            assert float(exempt_mask(x).mean()) <= EXEMPT_CAP, (it, k)
    assert EXEMPT_BELOW == 1e-6 and EXEMPT_CAP == 1e-3
    assert g["wp"].shape == (PROJ_B, 10, 512) and g["styles0"].shape == (PROJ_B * sum(S64_CHANNELS),)
    assert np.array_equal(g["it0_styles"], g["styles0"])
