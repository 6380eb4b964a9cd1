"""The four generator families behind one interface (E_align_s2.py:27-86, 102-162): what a training or inference step asks of
its generator.  `make_adapter` is the only place that looks at a generator's type; the steps call the adapter."""
import numpy as np
import torch

from .biggan_generator import BigGAN
from .pggan_generator import PGGANGenerator
from .stylegan2_generator import StyleGAN2Generator, mixing_mask


def set_seed(seed):
    """training_utils.py:46-52"""
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    from . import ops
    ops.noise_seed(seed)            # the step's device noise is counter-based: (seed, draw number, global element index)


def truncated_noise_sample(batch_size=1, dim_z=128, truncation=1.0, seed=None):
    """training_utils.py:32-44 (scipy truncnorm on a seeded RandomState)"""
    from scipy.stats import truncnorm
    state = None if seed is None else np.random.RandomState(seed)
    return truncation * truncnorm.rvs(-2, 2, size=(batch_size, dim_z), random_state=state).astype(np.float32)


class GeneratorAdapter:
    """Defaults of the interface.  `sample(z, noises)` -> (imgs1, w1) and `synth(w, noises)` -> imgs are the family's own;
    `encode(E, imgs1, noises)` -> (const2, w2)."""

    capturable = True         # an iteration can be captured into a hipGraph (its host decisions have device-input forms)
    prefetchable = True       # the pass that opens iteration n + 1 may be issued during iteration n
    conditional, flag = False, 0        # class-conditional: `flag` is the class id of the last draw, `const1` the encoder's condition
    new_z = None              # StyleGAN2 parity runs: the reference's own second latent of the style mixing (stylegan2_generator.py:187)

    def draw(self, iteration, n, z_dim):
        """host z of the GLOBAL batch, drawn behind set_seed (E_align_s2.py:103-104)"""
        return torch.randn(n, z_dim)

    def z_dim(self, default):
        return default

    def encode(self, E, imgs1, noises=None):
        return E(imgs1, noises=noises)

    def set_mixing_latent(self, new_z):
        pass

    def graph_inputs(self, device):
        """allocates the device inputs that replace the family's host decisions in a captured iteration"""

    def refresh_graph_inputs(self):
        """makes those decisions for the next replay, with the reference's draws in the reference's order"""


class StyleGAN2Adapter(GeneratorAdapter):
    """mtype 2: generator(z, trunc...) -> dict, generator.synthesis(wp) -> dict (E_align_s2.py:110-115,160)"""

    def __init__(self, generator):
        self.G = generator

    mix_mask = None          # device [L] mask: set in hipGraph mode (static kernel sequence)

    def sample(self, z, noises=None):
        r = self.G(z, trunc_psi=0.7, trunc_layers=8, randomize_noise=False, mix_mask=self.mix_mask, new_z=self.new_z)
        return r["image"], r["wp"]

    def synth(self, w, noises=None):
        return self.G.synthesis(w)["image"]

    def set_mixing_latent(self, new_z):
        self.new_z = new_z

    def graph_inputs(self, device):
        self.mix_mask = torch.zeros(self.G.num_layers, device=device)

    def refresh_graph_inputs(self):
        if self.mix_mask is not None:
            self.mix_mask.copy_(mixing_mask(self.G.num_layers))


class StyleGAN1Adapter(GeneratorAdapter):
    """mtype 1: w1 = Gm(z, coefs_m=coefs); imgs = Gs.forward(w, lod) with lod = log2(img_size)-2 (E_align_s2.py:27-41,105-108,158)"""

    def __init__(self, Gs, Gm):
        self.G, self.Gm = Gs, Gm
        n = 2 * Gs.layer_count
        layer_idx = torch.arange(n)[None, :, None]
        ones = torch.ones(layer_idx.shape, dtype=torch.float32)
        self.coefs = torch.where(layer_idx < n // 2, 0.7 * ones, ones)      # truncation psi on the first half of the layers
        self.lod = Gs.layer_count - 1

    def sample(self, z, noises=None):
        w1 = self.Gm(z, coefs_m=self.coefs)
        return self.G.forward(w1, self.lod, noises=noises), w1

    def synth(self, w, noises=None):
        return self.G.forward(w, self.lod, noises=noises)


class PGGANAdapter(GeneratorAdapter):
    """mtype 3: w1 = z; imgs1 = generator(w1)['image'] (E_align_s2.py:134-138).  The script's second pass calls
    `generator.synthesis(w2)` (:160), which PGGANGenerator does not have; the evident intent
    `generator(w2)['image']` is what runs here."""

    def __init__(self, generator):
        self.G = generator

    def sample(self, z, noises=None):
        return self.G(z)["image"], z

    def synth(self, w, noises=None):
        return self.G(w)["image"]


class BigGANAdapter(GeneratorAdapter):
    """mtype 4 (E_align_s2.py:139-150,155,162): z = 0.4 * truncnorm(seed), one class id per batch drawn with
    np.random.randint(1000) after set_seed, truncation = float32 tensor 0.4 (kept on the host: its BN-row arithmetic is the
    reference's float32 division); the encoder is conditioned on the generator's condition vector.  z is a scipy draw and the
    class id a host decision of every iteration: neither capture nor prefetch."""

    capturable = prefetchable = False
    conditional = True

    def __init__(self, generator):
        self.G = generator
        self.truncation = torch.tensor(0.4, dtype=torch.float)
        self.conditions = self.const1 = None

    def draw(self, iteration, n, z_dim=None):
        z = truncated_noise_sample(truncation=0.4, batch_size=n, dim_z=self.G.config.z_dim, seed=iteration % 30000)
        self.flag = int(np.random.randint(1000))
        return torch.tensor(z, dtype=torch.float)

    def z_dim(self, default):
        return self.G.config.z_dim

    def sample(self, z, noises=None):
        B = z.shape[0]
        self.conditions = torch.zeros(B, self.G.config.num_classes, device=z.device)
        self.conditions[:, self.flag] = 1.0
        imgs1, self.const1 = self.G(z, self.conditions, self.truncation)
        return imgs1, z

    def synth(self, w, noises=None):
        return self.G(w, self.conditions, self.truncation)[0]

    def encode(self, E, imgs1, noises=None):
        return E(imgs1, self.const1, noises=noises)


def generator_family(generator):
    """'pggan', 'biggan' or 'stylegan2' by the generator's class; None for anything else (a StyleGAN1 synthesis network, a stand-in)"""
    known = ((PGGANGenerator, "pggan"), (BigGAN, "biggan"), (StyleGAN2Generator, "stylegan2"))
    return next((name for cls, name in known if isinstance(generator, cls)), None)


def make_adapter(generator, mapping=None):
    """`generator`: StyleGAN2Generator (mtype 2), the StyleGAN1 synthesis network Gs together with `mapping` = Gm (mtype 1), a
    PGGANGenerator (mtype 3) or a BigGAN (mtype 4).  What is none of them is driven through StyleGAN2's interface."""
    if mapping is not None:
        return StyleGAN1Adapter(generator, mapping)
    return {"pggan": PGGANAdapter, "biggan": BigGANAdapter}.get(generator_family(generator), StyleGAN2Adapter)(generator)
