"""What the two-phase inversion steps share (embedding_v2.LatentEmbedStep with embedding_v2_pggan.PGEmbedStep, and
embedding_v2_biggan.BigEmbedStep with its rows form): the constructor tail, the start of an image group, the optimiser phase, the
tracker read-out and the hipGraph plumbing.  step() itself - the loss composition and the result keys - is each family's own.

A subclass provides `_latent_shape(B)`, `_start_code(imgs1, shape, noises, needed)`, where a group needs more than its images
(BigGAN's class conditions) `_begin_group(imgs1, **group_kw)`, and where it steps a second optimiser (the noise maps') its own
`_graph_opts()`."""
import os

import torch

from . import ops, weight_cache
from .custom_adam import LREQAdam
from .embed_track import EmbedTracker, tracker_rules
from .graph_step import GraphReplay


def several_processes(env=False):
    """True when torch.distributed runs more than one process; `env`: or WORLD_SIZE announces more than one (a launcher's CLI)."""
    dist = torch.distributed
    return (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1) or \
        (env and int(os.environ.get("WORLD_SIZE", "1")) > 1)


class TwoPhaseEmbedStep(GraphReplay):
    MODES = ("E", "W")

    def __init__(self, G, E, lpips_model, mode, kind, lr, beta_1, iterations, arm_iter=None, events_cap=256, independent=False):
        """The tail of a subclass constructor, behind its own argument checks: `kind` names the tracker rules.  Mode "E" gets the
        LREQAdam over the encoder and the checkpoint every group restarts from; every other mode freezes the encoder (whether E and
        G run in eval or train mode is the subclass's decision) and gets its optimiser with the leaf, in begin_image."""
        if mode not in self.MODES:
            names = [repr(m) for m in self.MODES]
            raise ValueError(f"mode must be {', '.join(names[:-1])} or {names[-1]}, got {mode!r}")
        self.G, self.E, self.lpips, self.mode = G, E, lpips_model, mode
        self.lr, self.beta_1, self.iterations = lr, beta_1, int(iterations)
        self.independent = bool(independent)
        self.rules = tracker_rules(kind, self.iterations)
        if arm_iter is not None:
            self.rules["arm_iter"] = int(arm_iter)
        self.events_cap = int(events_cap)
        self._tracker = EmbedTracker(self.rules, self.events_cap, rows=self.independent)
        self.group = -1
        self.last = {}
        self.w1 = None
        if mode == "E":
            self.opt = LREQAdam([{"params": E.parameters()}], lr=lr, betas=(beta_1, 0.99), weight_decay=0)
            self._ckpt = {k: v.detach().clone() for k, v in E.state_dict().items()}
        else:
            for p in E.parameters():          # frozen: the encoder backward computes the data gradient only
                p.requires_grad_(False)
            self.opt = None

    # ------------------------------------------------------------------ per image group
    def _begin_group(self, imgs1):
        pass

    def begin_image(self, imgs1, w_init=None, noises=None, **group_kw):
        """Start an image group.  Mode "E" re-loads the encoder checkpoint; every other mode copies the start code - `w_init`, else
        the subclass's - into the persistent leaf w1 (allocated once per shape and device: a captured iteration stays valid).  The
        Adam state is cleared and the tracker restarts, both in place.  `noises`: optional noise list of the start code's E(imgs1)
        (parity runs)."""
        dev = imgs1.device
        self._begin_group(imgs1, **group_kw)
        self.group += 1
        shape = self._latent_shape(imgs1.shape[0])
        if self.mode == "E":
            self.E.load_state_dict(self._ckpt)
            weight_cache.written(self.E.parameters())
        else:
            with torch.no_grad():
                w0 = self._start_code(imgs1, shape, noises, needed=w_init is None)
                if w_init is not None:
                    w0 = w_init.to(dev, torch.float32).reshape(shape)
                if self.w1 is None or tuple(self.w1.shape) != shape or self.w1.device != dev:
                    if self.captured:
                        raise ValueError(f"{type(self).__name__}.begin_image: the captured iteration works on a different latent shape")
                    self.w1 = torch.zeros(shape, dtype=torch.float32, device=dev, requires_grad=True)
                    self.opt = LREQAdam([{"params": [self.w1]}], lr=self.lr, betas=(self.beta_1, 0.99), weight_decay=0)
                self.w1.copy_(w0)
        self._reset_opt()
        self._tracker.reset(shape, dev)

    # ------------------------------------------------------------------ one optimiser phase of an iteration
    def _opt_phase(self, loss, retain_graph=False):
        self.opt.zero_grad()
        loss.backward(retain_graph=retain_graph)
        self.opt.step()

    # ------------------------------------------------------------------ hipGraph replay of the iteration
    def capture(self, imgs1, noises=(None, None, None), warmup=GraphReplay.WARMUP):
        """`warmup` real iterations, then one recorded (not executed) iteration (GraphReplay._capture).  Adam's step factors come
        through graph_advance, the noise seed is a device scalar; with a leaf w1 the graph updates it in place.  begin_image() must
        have run for the group."""
        self._g_imgs1 = imgs1.detach().clone()
        for opt, calls in self._graph_opts():
            opt.graph_begin(calls, imgs1.device)
        ops.noise_graph_begin(imgs1.device)
        self.graph_iteration = 0
        return self._capture_keeping_last(lambda: self.step(self._g_imgs1, noises), warmup)

    def _graph_opts(self):
        return [(self.opt, 2)]          # two optimizer calls per iteration

    def _graph_inputs(self, iteration):
        for opt, _ in self._graph_opts():
            opt.graph_advance()
        ops.noise_graph_seed(iteration)

    def set_image(self, imgs1):
        """Copies a new image group into the static input of the captured iteration (call begin_image() for the group too)."""
        self._set_static("_g_imgs1", imgs1)

    def replay(self):
        self.last = super().replay()
        return self.last

    # ------------------------------------------------------------------ tracker read-out (one host read)
    def tracker(self):
        """The tracker's state on the host; independent / rows form: a list with one such read-out per row."""
        return self._tracker.read()
