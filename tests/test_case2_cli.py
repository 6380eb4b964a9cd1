"""dge_amd.e_align_case2 without a GPU: the --preset table, Case2Step's argument validation, the C-ABI entry of the split
window-gradient kernel and the three reference fixtures."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import golden, ROOT

# (image phases, latent terms, latent scale) read off each script's loop body:
#   4.E_align_w_zn.py:72-90          loss_imgs step; loss_w * 0.01 (loss_c commented out)
#   5.E_align_w_zn_zc.py:73-91       loss_imgs step; (loss_w + loss_c) * 0.01
#   6.E_align_x.py:73-91             loss_imgs step; (loss_w + loss_c) * 0.01
#   7.E_align_x_AT1.py:73-99         loss_imgs step, 5 * loss_medium step; (loss_w + loss_c) * 0.01
#   8.E_align_x_AT1_AT2.py:73-117    loss_imgs, 5 * loss_medium, 9 * loss_small steps; (loss_w + loss_c) * 0.01
#   Cat256/E_align_case_2.py:185-228 the three image steps; loss_w.backward() alone, unscaled (loss_c is logged only)
TABLE = {
    "ablation4": (("imgs",), ("w",), 0.01),
    "ablation5": (("imgs",), ("w", "c"), 0.01),
    "ablation6": (("imgs",), ("w", "c"), 0.01),
    "ablation7": (("imgs", "AT1"), ("w", "c"), 0.01),
    "ablation8": (("imgs", "AT1", "AT2"), ("w", "c"), 0.01),
    "cat256": (("imgs", "AT1", "AT2"), ("w",), 1.0),
}


@pytest.mark.parametrize("preset", sorted(TABLE))
def test_preset_expands_to_the_scripts_loop_body(preset):
    from dge_amd import e_align_case2 as C2
    args = C2.build_parser().parse_args(["--preset", preset, "--mtype", "2" if preset == "cat256" else "1"])
    assert C2.resolve_recipe(args) == TABLE[preset]
    assert set(C2.PRESETS) == set(TABLE)


def test_explicit_flags_override_the_preset_and_defaults_follow_mtype():
    from dge_amd import e_align_case2 as C2
    p = C2.build_parser()
    assert C2.resolve_recipe(p.parse_args(["--preset", "ablation8", "--phases", "imgs,AT2", "--latent", "w", "--latent_scale", "0.5"])) == \
        (("imgs", "AT2"), ("w",), 0.5)
    assert C2.resolve_recipe(p.parse_args([])) == TABLE["ablation8"]
    assert C2.resolve_recipe(p.parse_args(["--mtype", "2"])) == TABLE["cat256"]
    with pytest.raises(SystemExit):
        C2.main(["--mtype", "3", "--iterations", "0"])


class _Gs(torch.nn.Module):            # stands in for the StyleGAN1 synthesis network: the adapter reads layer_count only
    layer_count = 5

    def __init__(self):
        super().__init__()
        self.const = torch.nn.Parameter(torch.ones(1, 64, 4, 4))


def _blur():
    from dge_amd.encoder_variants import BlurBE
    return BlurBE(startf=16, maxf=64, layer_count=5, compute_dtype="f32")


def test_case2step_accepts_the_supported_forms_on_stub_modules():
    from dge_amd.e_align_case2 import Case2Step
    st = Case2Step(_Gs(), _blur(), None, mapping=torch.nn.Identity(), image_phases=("AT2", "imgs"), latent_terms=("c", "w"))
    assert st.image_phases == ("imgs", "AT2") and st.latent_terms == ("w", "c")          # the scripts' order
    with pytest.raises(RuntimeError, match="eager"):
        st.capture()
    with pytest.raises(ValueError, match="prefetch_next"):
        st.step(0, prefetch_next=True)


@pytest.mark.parametrize("kw,exc,msg", [
    (dict(image_phases=()), ValueError, "empty"),
    (dict(image_phases=("imgs", "imgs")), ValueError, "twice"),
    (dict(image_phases=("imgs", "AT3")), ValueError, "unknown"),
    (dict(latent_terms=()), ValueError, "empty"),
    (dict(latent_terms=("w", "z")), ValueError, "unknown"),
    (dict(latent_terms=("w", "w")), ValueError, "twice"),
])
def test_case2step_rejects_bad_phase_names(kw, exc, msg):
    from dge_amd.e_align_case2 import Case2Step
    with pytest.raises(exc, match=msg):
        Case2Step(_Gs(), _blur(), None, mapping=torch.nn.Identity(), **kw)


def test_case2step_rejects_unsupported_models():
    from dge_amd.e_align_case2 import Case2Step
    from dge_amd.encoder import BE
    from dge_amd.pggan_generator import PGGANGenerator
    from dge_amd.stylegan2_generator import StyleGAN2Generator
    with pytest.raises(ValueError, match="E_Blur"):
        Case2Step(_Gs(), BE(startf=16, maxf=64, layer_count=5, compute_dtype="f32"), None, mapping=torch.nn.Identity())
    with pytest.raises(ValueError, match="mtype 3"):
        Case2Step(PGGANGenerator(resolution=64, compute_dtype="f32"), _blur(), None)
    with pytest.raises(ValueError, match="mapping=Gm"):
        Case2Step(_Gs(), _blur(), None)
    G2 = StyleGAN2Generator(64, fmaps_base=2048, fmaps_max=128, compute_dtype="f32")
    with pytest.raises(ValueError, match="loss_w alone"):
        Case2Step(G2, _blur(), None)                                   # default latent terms include 'c'
    Case2Step(G2, _blur(), None, latent_terms=("w",), latent_scale=1.0)


def test_case2step_rejects_a_data_parallel_run(monkeypatch):
    import torch.distributed as dist
    from dge_amd.e_align_case2 import Case2Step
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    try:
        with pytest.raises(RuntimeError, match="single process"):
            Case2Step(_Gs(), _blur(), None, mapping=torch.nn.Identity())
    finally:
        from dge_amd import ops
        ops.noise_dp(0, 1)


def test_library_exports_the_split_kernel_entry():
    import ctypes
    from dge_amd import _lib
    assert len(_lib.SIGNATURES["dge_space_loss_bwd_split"]) == len(_lib.SIGNATURES["dge_space_loss_bwd3"]) == 14
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dge_space_loss_bwd_split")
    with open(os.path.join(ROOT, "include", "dge_hip.h")) as f:
        assert "int dge_space_loss_bwd_split(" in f.read()


_PARAMS = ("decode_block.0.conv_1.weight", "decode_block.3.conv_2.weight", "decode_block.4.inver_mod2.weight", "decode_block.1.bias_1",
           "FromRGB.from_rgb.weight")


@pytest.mark.parametrize("name,nphase,full", [("step_case2_sg1.npz", 4, True), ("step_case2_s2.npz", 4, True), ("step_case2_sub.npz", 2, False)])
def test_case2_goldens_have_the_documented_keys(name, nphase, full):
    g = golden(name)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "step_big.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) <= 1 << 20
    for it in range(2):
        need = [f"it{it}_losses", f"it{it}_param_checksum"] + [f"it{it}_after_phase{ph}:{k}" for ph in range(1, nphase + 1) for k in _PARAMS]
        if full:
            need += [f"it{it}_{k}" for k in ("w1", "imgs1", "w2", "imgs2", "const2", "info")]
        for k in need:
            assert k in g.files and k + "_ref_spread" in g.files, k
            assert np.isfinite(g[k]).all() and 0 <= float(g[k + "_ref_spread"]) < 1e-4, k
        assert f"it{it}_after_phase{nphase + 1}:{_PARAMS[0]}" not in g.files
        assert g[f"it{it}_losses"].shape == (6,)
    assert tuple(g["noise_split"].shape) == (2,) and int(g["noise_split"].sum()) <= len(g["noise_shapes"])
