"""CPU checks of the Z-space encoder training entry points (dge_amd.e_align_z, reference ablation_utils/1.E_align_z.py)."""
import json
import os

import pytest

from tests.conftest import ROOT


def test_cli_defaults_equal_the_reference():
    from dge_amd.e_align_z import build_parser
    a = build_parser().parse_args([])
    ref = {"iterations": 60001, "lr": 0.0015, "beta_1": 0.0, "batch_size": 2, "experiment_dir": None,   # 1.E_align_z.py:137-149
           "checkpoint_dir_GAN": "../checkpoint/stylegan_v1/ffhq1024/",
           "config_dir": "./checkpoint/biggan/256/biggan-deep-256-config.json", "checkpoint_dir_E": None, "img_size": 1024,
           "img_channels": 3, "z_dim": 512, "mtype": 1, "start_features": 16}
    assert {k: getattr(a, k) for k in ref} == ref


@pytest.mark.parametrize("mtype", ["2", "3", "4"])
def test_other_model_types_are_refused(mtype, capsys):
    from types import SimpleNamespace
    from dge_amd.e_align_z import main, load_models
    with pytest.raises(SystemExit):
        main(["--mtype", mtype])
    assert "error" in capsys.readouterr().out
    with pytest.raises(ValueError, match="mtype 1"):
        load_models(SimpleNamespace(mtype=int(mtype)))


def test_e_blur_z_state_dict_matches_reference_keys():
    from dge_amd.encoder_variants import BlurBEZ
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "encz_keys.json")))
    sd = BlurBEZ(startf=32, maxf=512, layer_count=5, compute_dtype="f32").state_dict()
    assert list(sd.keys()) == list(ref.keys())
    assert all(list(sd[k].shape) == ref[k] for k in sd)
    E = BlurBEZ(startf=32, maxf=512, layer_count=5, compute_dtype="f32")
    assert not any("noise_weight" in k or "inver_mod" in k for k in E.state_dict())
    assert getattr(E.out_z.weight, "lr_equalization_coef") == pytest.approx(2 ** 0.5 / (9 * 512) ** 0.5)
    assert getattr(E.out_z.bias, "lr_equalization_coef") == 1.0
    assert len(BlurBEZ(startf=16, maxf=512, layer_count=9).state_dict()) > 0      # FFHQ-1024, the reference's default


def test_e_blur_z_width_checks():
    from dge_amd.encoder_variants import BlurBEZ
    with pytest.raises(ValueError, match="must not change width"):
        BlurBEZ(startf=16, maxf=512, layer_count=5)         # last block 256 -> 512
    with pytest.raises(ValueError, match="512 channels"):
        BlurBEZ(startf=32, maxf=256, layer_count=5)         # last block 256 -> 256, out_z wants 512


def test_mapping_backward_is_in_the_c_abi():
    from dge_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dge_hip.h")).read()
    assert "int dge_mapping_bwd(" in hdr and "dge_mapping_bwd" in _lib.SIGNATURES
