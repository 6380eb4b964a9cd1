"""tests/golden/s2_mapping_grad.npz (tools/gen_golden_s2_mapping.py: the reference StyleGAN2 mapping and truncation with their z
gradients) against a float64 numpy restatement of pixel norm, the dense chain, the truncation and the adjoint - the restatement
the GPU tests of dge_mapping_bwd_wide use as their exact arithmetic (mapping_fwd_ref / mapping_bwd_ref)."""
import numpy as np
import pytest

from tests.conftest import golden

ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2          # ops.ACT_* (include/dge_hip.h)


def dense_layer(w, b, wscale=1.0, bscale=1.0, add=0.0, act=ACT_LRELU, gain=1.0):
    return dict(w=np.asarray(w, np.float64), b=None if b is None else np.asarray(b, np.float64), wscale=float(wscale), bscale=float(bscale),
                add=float(add), act=int(act), gain=float(gain))


def mapping_fwd_ref(z, layers, pixelnorm=True, eps=1e-8):
    """(chain input, [output of every layer]) in float64: y = act((x W^T)*wscale + b*bscale + add)*gain, leaky-relu slope 0.2."""
    x = np.asarray(z, np.float64)
    if pixelnorm:
        x = x / np.sqrt((x * x).mean(axis=1, keepdims=True) + eps)
    x0, acts = x, []
    for Ly in layers:
        v = x @ Ly["w"].T * Ly["wscale"] + (0.0 if Ly["b"] is None else Ly["b"] * Ly["bscale"]) + Ly["add"]
        if Ly["act"] == ACT_LRELU:
            v = np.where(v > 0, v, 0.2 * v)
        elif Ly["act"] == ACT_RELU:
            v = np.maximum(v, 0.0)
        x = v * Ly["gain"]
        acts.append(x)
    return x0, acts


def mapping_bwd_ref(z, layers, g, coefs=None, acts=None, pixelnorm=True, eps=1e-8):
    """dge_mapping_bwd's contract in float64: sum_l coefs[l]*g[b,l,:], the transposed chain (the activation slope read off the
    layer OUTPUT `acts[l]`: 1 where it is > 0, else 0.2 / 0 - an output of exactly 0 takes the negative side), the pixel-norm
    adjoint.  acts None: the float64 forward's."""
    z = np.asarray(z, np.float64)
    if acts is None:
        acts = mapping_fwd_ref(z, layers, pixelnorm, eps)[1]
    g = np.asarray(g, np.float64)
    c = np.ones(g.shape[1]) if coefs is None else np.asarray(coefs, np.float64).reshape(-1)
    gr = (g * c[None, :, None]).sum(axis=1)
    for Ly, h in zip(reversed(layers), reversed(acts)):
        h = np.asarray(h, np.float64)
        slope = {ACT_LRELU: np.where(h > 0, 1.0, 0.2), ACT_RELU: np.where(h > 0, 1.0, 0.0), ACT_NONE: np.ones_like(h)}[Ly["act"]]
        gr = (gr * (Ly["gain"] * slope * Ly["wscale"])) @ Ly["w"]
    if not pixelnorm:
        return gr
    I0 = z.shape[1]
    r = 1.0 / np.sqrt((z * z).mean(axis=1, keepdims=True) + eps)
    return r * gr - z * (r ** 3 / I0) * (gr * z).sum(axis=1, keepdims=True)


def truncation_ref(w, w_avg, L, psi, layers):
    """(wp [B, L, D], coefs [L] or None): the reference's TruncationModule on a [B, D] code."""
    wp = np.repeat(np.asarray(w, np.float64)[:, None, :], L, axis=1)
    psi = 1.0 if psi is None else psi
    layers = 0 if layers is None else layers
    if not (psi < 1.0 and layers > 0):
        return wp, None
    c = np.where(np.arange(L) < layers, psi, 1.0)
    avg = np.asarray(w_avg, np.float64)[None, None, :]
    return avg + (wp - avg) * c[None, :, None], c


def s2z_mapping_layers():
    """The eight DenseBlocks of tests/s2z_models.py's generator as restatement entries (reference :925-996: wscale = lr_mul /
    sqrt(I), bscale = lr_mul, leaky-relu 0.2 with gain sqrt 2)."""
    from tests.s2z_models import MAPPING_LR_MUL, s2z_state_dict
    sd = s2z_state_dict()
    out = []
    for i in range(8):
        w = sd[f"mapping.dense{i}.weight"].numpy()
        out.append(dense_layer(w, sd[f"mapping.dense{i}.bias"].numpy(), MAPPING_LR_MUL / np.sqrt(w.shape[1]), MAPPING_LR_MUL,
                               0.0, ACT_LRELU, np.sqrt(2.0)))
    return out


def maxrel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def restated():
    from tests.golden import recipe as R
    g = golden("s2_mapping_grad.npz")
    layers = s2z_mapping_layers()
    z = g["z"]
    assert np.array_equal(z, R.randn("s2map.z", (3, 512), int(g["z_seed"])).numpy())
    return g, layers, z, mapping_fwd_ref(z, layers)[1]


def test_fixture_w_matches_the_float64_restatement(restated):
    g, layers, z, acts = restated
    assert maxrel(acts[-1], g["w"]) < 1e-6
    assert float(np.abs(g["w"]).max()) > 1.0 and float(g["kink_margin"]) > 2e-5          # a live mapping, clear of the leaky-relu kinks


@pytest.mark.parametrize("tag,psi,layers_t", [("t8", 0.7, 8), ("t10", 0.7, 10), ("none", None, None)])
def test_fixture_wp_and_dz_match_the_float64_restatement(restated, tag, psi, layers_t):
    from tests.golden import recipe as R
    g, layers, z, acts = restated
    wp, coefs = truncation_ref(acts[-1], g["w_avg"], 10, psi, layers_t)
    assert (coefs is None) == (tag == "none")
    assert maxrel(wp, g["wp_" + tag]) < 1e-6
    gw = R.randn("s2map.gw." + tag, (3, 10, 512), 82).numpy()
    dz = mapping_bwd_ref(z, layers, gw, coefs)
    assert float(np.abs(g["dz_" + tag]).max()) > 1.0
    assert maxrel(dz, g["dz_" + tag]) < 1e-6
