"""The three training parsers (dge_amd.e_align, e_align_z, e_align_case2) share models.add_train_args / add_model_args: with no
arguments each yields exactly the defaults it had when it spelled every flag out itself (the reference scripts' values)."""
import pytest

_COMMON = {"lr": 0.0015, "beta_1": 0.0, "batch_size": 2, "experiment_dir": None, "checkpoint_dir_E": None, "img_size": 1024,
           "img_channels": 3, "z_dim": 512, "start_features": 16, "compute_dtype": "bf16", "vgg_weights": None, "lpips_weights": None,
           "deterministic": False, "allow_standin_lpips": False, "fmaps_base": None, "fmaps_max": None, "enc_maxf": None}

DEFAULTS = {
    "e_align": dict(_COMMON, iterations=210000, checkpoint_dir_GAN=None, config_dir=None, mtype=2, launch="auto", no_prefetch=False,
                    stage=2, legacy_zero_grad=False),
    # (fmaps_base / fmaps_max / enc_maxf: new with the shared model flags, None, not passed on)
    "e_align_z": dict(_COMMON, iterations=60001, checkpoint_dir_GAN="../checkpoint/stylegan_v1/ffhq1024/",
                      config_dir="./checkpoint/biggan/256/biggan-deep-256-config.json", mtype=1),
    "e_align_case2": dict(_COMMON, iterations=60001, checkpoint_dir_GAN=None, config_dir=None, mtype=1, preset=None, phases=None,
                          latent=None, latent_scale=None),
}


@pytest.mark.parametrize("module", sorted(DEFAULTS))
def test_parser_defaults_are_unchanged(module):
    import importlib
    args = importlib.import_module("dge_amd." + module).build_parser().parse_args([])
    assert vars(args) == DEFAULTS[module]
