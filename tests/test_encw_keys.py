"""E_Blur_W / E_Blur_W_2 (encoder_variants.BlurBEW, BlurBEW2) without a GPU: state_dict keys and shapes against the reference's
(tests/golden/encw_keys.json, tools/gen_golden.py section encw_grad), strict loading, and what the classes declare."""
import json
import os

import pytest
import torch

from tests.conftest import ROOT
from tests.golden import recipe as R

KEYS = json.load(open(os.path.join(ROOT, "tests", "golden", "encw_keys.json")))
CONFIGS = [(1024, 16, 9), (256, 64, 7)]


def _cls(variant):
    from dge_amd.encoder_variants import BlurBEW, BlurBEW2
    return {"w": BlurBEW, "w_2": BlurBEW2}[variant]


@pytest.mark.parametrize("variant", ["w", "w_2"])
@pytest.mark.parametrize("size,startf,L", CONFIGS)
def test_state_dict_matches_reference_keys_in_order_and_loads_strict(variant, size, startf, L):
    ref = KEYS[f"{variant}:{size}/{startf}/{L}"]
    E = _cls(variant)(startf=startf, maxf=512, layer_count=L, compute_dtype="f32")
    sd = E.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    assert all(list(sd[k].shape) == ref[k] for k in sd)
    assert not any("noise_weight" in k for k in sd)
    assert sum("inver_mod1" in k for k in sd) == 2 * L and sum("inver_mod2" in k for k in sd) == 2 * L
    # a reference-shaped state_dict (as torch.save(E.state_dict()) of the scripts writes it) loads with strict=True
    filled = R.fill_encoder(ref, seed=5)
    E.load_state_dict(filled, strict=True)
    assert torch.equal(E.decode_block[L - 1].inver_mod2.weight.detach(), filled[f"decode_block.{L - 1}.inver_mod2.weight"])


def test_the_two_reference_encoders_have_the_same_keys():
    for size, startf, L in CONFIGS:
        assert KEYS[f"w:{size}/{startf}/{L}"] == KEYS[f"w_2:{size}/{startf}/{L}"]


def test_declarations():
    from dge_amd.encoder_variants import BlurBE, BlurBEW, BlurBEW2
    assert BlurBEW.noise is False and BlurBEW2.noise is False
    assert BlurBEW.w_rows == {"inver_mod1": (1,), "inver_mod2": (0,)}          # w_ = cat(w2, w1)
    assert BlurBEW2.w_rows == {"inver_mod2": (0, 1)}                            # w_ = cat(w2, w2): inver_mod1 feeds nothing
    assert not hasattr(BlurBE, "w_rows")                                        # E_Blur keeps its per-head launches
    E = BlurBEW2(startf=32, maxf=512, layer_count=5, compute_dtype="f32")
    assert getattr(E.decode_block[0].inver_mod1.weight, "lr_equalization_coef") == getattr(E.decode_block[0].inver_mod2.weight, "lr_equalization_coef")
    with pytest.raises(ValueError, match="block_num"):
        E(torch.zeros(1, 3, 64, 64), block_num=8)
    with pytest.raises(ValueError, match="draws no noise"):
        E(torch.zeros(1, 3, 64, 64), noises=[torch.zeros(1)])


@pytest.mark.parametrize("variant,cls", [(None, "BlurBE"), ("z", "BlurBEZ"), ("w", "BlurBEW"), ("w_2", "BlurBEW2")])
def test_models_blur_encoder_selects_the_variant(variant, cls):
    from dge_amd import models
    E = models.blur_encoder(1024, 16, "bf16", "cpu", variant=variant)
    assert type(E).__name__ == cls and E.layer_count == 9
    with pytest.raises(ValueError, match="unknown variant"):
        models.blur_encoder(256, 64, "bf16", "cpu", variant="w_3")
    assert type(models.blur_encoder(1024, 16, "bf16", "cpu", z_space=True)).__name__ == "BlurBEZ"


def test_grouped_head_kernels_are_in_the_c_abi():
    from dge_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dge_hip.h")).read()
    for name in ("dge_heads_rows_fwd", "dge_heads_rows_bwd", "dge_head_rows_entry_size"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES
    # the one-column head kernels keep their ABI
    assert _lib.SIGNATURES["dge_heads_fwd"] == [_lib._P, _lib._I, _lib._P, _lib._P, _lib._I, _lib._I, _lib._I, _lib._P]
    assert len(_lib.SIGNATURES["dge_heads_bwd"]) == 12
