"""The generator adapters' contract (dge_amd.generators) on stand-in generators: no library call, no GPU."""
from types import SimpleNamespace

import numpy as np
import torch

from dge_amd import generators as GEN
from dge_amd.biggan_generator import BigGAN
from dge_amd.pggan_generator import PGGANGenerator
from dge_amd.stylegan2_generator import StyleGAN2Generator


def _bare(cls, **attrs):
    """an instance of a generator class without its constructor: the factory looks at the type only"""
    g = cls.__new__(cls)
    torch.nn.Module.__init__(g)
    g.__dict__.update(attrs)
    return g


def _adapters():
    return {
        "stylegan1": GEN.make_adapter(SimpleNamespace(layer_count=5), mapping=torch.nn.Identity()),
        "stylegan2": GEN.make_adapter(_bare(StyleGAN2Generator, num_layers=10)),
        "pggan": GEN.make_adapter(_bare(PGGANGenerator)),
        "biggan": GEN.make_adapter(_bare(BigGAN, config=SimpleNamespace(z_dim=8, num_classes=1000))),
    }


def test_make_adapter_returns_the_family_adapter():
    a = _adapters()
    want = {"stylegan1": GEN.StyleGAN1Adapter, "stylegan2": GEN.StyleGAN2Adapter, "pggan": GEN.PGGANAdapter, "biggan": GEN.BigGANAdapter}
    assert {k: type(v) for k, v in a.items()} == want
    assert type(GEN.make_adapter(torch.nn.Identity())) is GEN.StyleGAN2Adapter          # a stand-in: StyleGAN2's interface
    for k, v in a.items():
        assert (v.capturable, v.prefetchable) == ((False, False) if k == "biggan" else (True, True)), k
        assert v.z_dim(512) == (8 if k == "biggan" else 512), k
    assert torch.equal(a["stylegan1"].coefs.flatten(), torch.tensor([0.7] * 5 + [1.0] * 5))


def test_default_draw_is_one_randn_of_the_global_batch():
    for k, v in _adapters().items():
        if k == "biggan":
            continue
        torch.manual_seed(7)
        z = v.draw(3, 4, 8)
        torch.manual_seed(7)
        assert torch.equal(z, torch.randn(4, 8)), k


def test_biggan_draw_takes_one_class_id_from_numpy():
    big = _adapters()["biggan"]
    np.random.seed(11)
    z = big.draw(5, 4, 512)
    after = np.random.randint(1 << 30)
    np.random.seed(11)
    flag = int(np.random.randint(1000))
    assert after == np.random.randint(1 << 30) and big.flag == flag
    assert tuple(z.shape) == (4, 8) and z.dtype == torch.float32 and float(z.abs().max()) <= 0.8
    assert np.array_equal(z.numpy(), GEN.truncated_noise_sample(truncation=0.4, batch_size=4, dim_z=8, seed=5))


def test_only_stylegan2_keeps_a_mixing_latent_and_a_mixing_mask():
    for k, v in _adapters().items():
        v.set_mixing_latent("nz")
        v.graph_inputs(torch.device("cpu"))
        assert v.new_z == ("nz" if k == "stylegan2" else None), k
        assert (getattr(v, "mix_mask", None) is not None) == (k == "stylegan2"), k
    m = _adapters()["stylegan2"]
    m.refresh_graph_inputs()                      # no captured iteration: nothing to refresh, no draw
    m.graph_inputs(torch.device("cpu"))
    np.random.seed(3)
    m.refresh_graph_inputs()
    assert tuple(m.mix_mask.shape) == (10,) and set(m.mix_mask.tolist()) <= {0.0, 1.0}
