"""What the encoder-training steps share (EAlignStep, MisAlignStep, Case2Step, EAlignZStep): the models behind a generator
adapter, the LREQAdam optimizer, the upload of z and the head of an iteration (E_align_s2.py:102-162): set_seed -> global z ->
this rank's rows -> device -> G(z) under no_grad -> encoder noise -> E(imgs1) -> G.synthesis(w2).  A step class differs in the
hooks `_first_pass` and `_encoder_noises`, and in what it does with the head's results."""
import torch

from . import ops
from .custom_adam import LREQAdam
from .generators import make_adapter, set_seed


class TrainStep:
    world, rank = 1, 0          # a data-parallel step class sets its own

    def __init__(self, generator, E, lpips_model, mapping=None, lr=0.0015, beta_1=0.0, batch_size=2, z_dim=512, reference_noise=False):
        """`generator`, `mapping`: see generators.make_adapter (a BigGAN's z_dim is taken from its config).
        `reference_noise`: encoder noise drawn on the CPU in the reference's order (Q6) instead of the device generator's."""
        self.G, self.E, self.lpips = generator, E, lpips_model
        self.gen = make_adapter(generator, mapping)
        self.opt = LREQAdam([{"params": E.parameters()}], lr=lr, betas=(beta_1, 0.99), weight_decay=0)
        self.batch_size, self.z_dim = batch_size, self.gen.z_dim(z_dim)
        self.reference_noise = reference_noise
        self.dev = next(E.parameters()).device
        self.last = {}
        ops.noise_dp(self.rank, self.world)      # device noise = this rank's rows of the global-batch draw

    @staticmethod
    def det(t):
        """(results are handed out detached: one that kept its grad_fn would keep the iteration's autograd graph alive, see EAlignStep.capture)"""
        return t.detach() if torch.is_tensor(t) else t

    def _upload(self, t):
        """Host tensor -> device without stalling the host: `t.to(device)` from pageable memory waits for the stream to drain
        (the whole previous step), after which the GPU idles until the host has queued work again.  z (drawn on the CPU after
        set_seed, like the reference, E_align_s2.py:103-104) goes through a small ring of pinned staging buffers instead; a
        buffer is reused only after the copy that read it has completed."""
        if t.is_cuda:
            return t.to(self.dev)
        ring = self.__dict__.setdefault("_pin_ring", {"i": 0, "slots": [None] * 4})
        k = ring["i"] = (ring["i"] + 1) % len(ring["slots"])
        slot = ring["slots"][k]
        if slot is None or slot[0].shape != t.shape or slot[0].dtype != t.dtype:
            slot = ring["slots"][k] = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True), None]
        if slot[1] is not None:
            slot[1].synchronize()
        slot[0].copy_(t)
        out = slot[0].to(self.dev, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        return out

    def _draw_z(self, iteration):
        """set_seed, then this rank's rows of the global z: every rank draws the same global batch and takes its slice"""
        B = self.batch_size
        set_seed(iteration % 30000)
        return self.gen.draw(iteration, B * self.world, self.z_dim)[self.rank * B:(self.rank + 1) * B]

    def _z_on_device(self, iteration, z):
        if z is None:
            z = self._draw_z(iteration)
        elif not z.is_cuda:
            set_seed(iteration % 30000)          # (a given host z: the iteration's other draws still follow the seed)
        return self._upload(z)

    def _first_pass(self, iteration, z, gen_noise):
        """z on the device and the generator pass under no_grad -> (z, imgs1, w1)"""
        z = self._z_on_device(iteration, z)
        with torch.no_grad():
            imgs1, w1 = self.gen.sample(z, gen_noise)
        return z, imgs1, w1

    def _encoder_noises(self, R):
        """reference_noise: the encoder's noise tensors for R x R images, drawn on the CPU in the reference's order"""
        from .enc_steps import draw_noises
        return [n.to(self.dev) for n in draw_noises(self.E, self.batch_size, R, "cpu")]

    def _head(self, iteration, z, noises, gen_noises, new_z, *, synth_grad=True):
        """-> z, imgs1, w1, const2, w2, imgs2.  `synth_grad=False`: the second pass runs under no_grad on a detached w2."""
        self.gen.set_mixing_latent(new_z)
        ops.zero_arena_begin(self.dev)       # one memset for all of this step's accumulation buffers
        z, imgs1, w1 = self._first_pass(iteration, z, gen_noises[0])
        if noises is None and self.reference_noise:
            noises = self._encoder_noises(imgs1.shape[2])
        const2, w2 = self.gen.encode(self.E, imgs1, noises)
        if synth_grad:
            imgs2 = self.gen.synth(w2, gen_noises[1])
        else:
            with torch.no_grad():
                imgs2 = self.gen.synth(w2.detach(), gen_noises[1])
        return z, imgs1, w1, const2, w2, imgs2
