"""CPU checks of the entry points of ablations 3 and 2 (dge_amd.e_align_w; reference ablation_utils/3.E_align_w.py, 2.E_align_w_2.py)."""
import pytest
import torch


def test_cli_defaults_equal_the_reference():
    from dge_amd.e_align_w import build_parser
    a = build_parser().parse_args([])
    ref = {"iterations": 60001, "lr": 0.0015, "beta_1": 0.0, "batch_size": 2, "experiment_dir": None,   # 3.E_align_w.py:135-148
           "checkpoint_dir_GAN": "../checkpoint/stylegan_v1/ffhq1024/",
           "config_dir": "./checkpoint/biggan/256/biggan-deep-256-config.json", "checkpoint_dir_E": None, "img_size": 1024,
           "img_channels": 3, "z_dim": 512, "mtype": 1, "start_features": 16}
    assert {k: getattr(a, k) for k in ref} == ref
    assert a.variant == "w"
    assert build_parser().parse_args(["--variant", "w_2"]).variant == "w_2"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--variant", "z"])


@pytest.mark.parametrize("mtype", ["2", "3", "4"])
def test_other_model_types_are_refused(mtype, capsys):
    from types import SimpleNamespace
    from dge_amd.e_align_w import main, load_models
    with pytest.raises(SystemExit) as e:
        main(["--mtype", mtype])
    assert e.value.code == 2
    assert "error" in capsys.readouterr().out
    with pytest.raises(ValueError, match="mtype 1"):
        load_models(SimpleNamespace(mtype=int(mtype), variant="w"))


def test_variant_selects_the_encoder_class():
    from dge_amd import e_align_w as W
    from dge_amd.encoder_variants import BlurBEW, BlurBEW2
    assert W.encoder_class("w") is BlurBEW and W.encoder_class("w_2") is BlurBEW2
    with pytest.raises(ValueError, match="unknown variant"):
        W.encoder_class("w_3")
    assert W.VARIANTS == ("w", "w_2")


class _Gs(torch.nn.Module):            # stands in for the StyleGAN1 synthesis network: the adapter reads layer_count only
    layer_count = 5

    def __init__(self):
        super().__init__()
        self.const = torch.nn.Parameter(torch.ones(1, 64, 4, 4))


@pytest.mark.parametrize("variant", ["w", "w_2"])
def test_step_is_the_case2_iteration_of_scripts_3_and_2(variant):
    from dge_amd.e_align_case2 import Case2Step
    from dge_amd.e_align_w import EAlignWStep, encoder_class
    E = encoder_class(variant)(startf=16, maxf=64, layer_count=5, compute_dtype="f32")
    st = EAlignWStep(_Gs(), torch.nn.Identity(), E, None)
    assert isinstance(st, Case2Step) and type(st).step is Case2Step.step          # the loop is reused, not copied
    assert st.image_phases == ("imgs",) and st.latent_terms == ("w",) and st.latent_scale == 0.01
    assert st._encoder_noises(64) is None                                          # nothing to replay
    with pytest.raises(RuntimeError, match="eager"):
        st.capture()
    # Case2Step itself accepts the two encoders
    Case2Step(_Gs(), E, None, mapping=torch.nn.Identity(), image_phases=("imgs",), latent_terms=("w",))


def test_encoder_checks():
    from dge_amd.e_align_case2 import Case2Step
    from dge_amd.e_align_w import EAlignWStep
    from dge_amd.encoder import BE
    from dge_amd.encoder_variants import BlurBE
    with pytest.raises(ValueError, match="E_Blur"):
        Case2Step(_Gs(), BE(startf=16, maxf=64, layer_count=5, compute_dtype="f32"), None, mapping=torch.nn.Identity())
    with pytest.raises(ValueError, match="E_Blur_W"):
        EAlignWStep(_Gs(), torch.nn.Identity(), BlurBE(startf=16, maxf=64, layer_count=5, compute_dtype="f32"), None)
    with pytest.raises(ValueError, match="E_Blur_W"):
        EAlignWStep(_Gs(), torch.nn.Identity(), BE(startf=16, maxf=64, layer_count=5, compute_dtype="f32"), None)


def test_presets_are_unchanged():
    from dge_amd.e_align_case2 import PRESETS
    assert PRESETS == {
        "ablation4": (("imgs",), ("w",), 0.01),
        "ablation5": (("imgs",), ("w", "c"), 0.01),
        "ablation6": (("imgs",), ("w", "c"), 0.01),
        "ablation7": (("imgs", "AT1"), ("w", "c"), 0.01),
        "ablation8": (("imgs", "AT1", "AT2"), ("w", "c"), 0.01),
        "cat256": (("imgs", "AT1", "AT2"), ("w",), 1.0),
    }
