"""E_align stage-2 encoder training step (reference E_align_s2.py:23-299) on the HIP path.

`EAlignStep.step()` is one iteration of the reference's hot loop (:102-221) for mtype 2
(StyleGAN2): seed -> z -> G (no grad, train-mode quirks kept) -> E -> G.synthesis (grad) ->
loss_imgs + 5*loss_medium + 9*loss_small -> backward(retain_graph) -> LREQAdam.step ->
0.01*loss_w -> backward -> step.  One process per GPU; with torch.distributed initialised the
encoder gradients are all-reduced over RCCL once per phase (flat 97 MB bucket at FFHQ-1024) and
the batch-coupled loss terms (cosine, means) use globally reduced sums so that N ranks x B
images reproduce a single-process run at batch N*B.
"""
import os

import torch
import torch.distributed as dist

from . import losses, ops
from .collectives import GradBucket
from .generators import set_seed, truncated_noise_sample  # noqa: F401  (both re-exported: tests and tools import them from here)
from .graph_step import GraphReplay
from .models import (add_model_args, add_train_args, build_models, build_models_big, build_models_pg,  # noqa: F401  (re-exported)
                     build_models_sg1, imgs_px, load_lpips_weights, load_models, prepare_training)
from .train_step import TrainStep
from .weight_cache import pack_cache, refresh_packs


class EAlignStep(TrainStep, GraphReplay):
    comm_stats = None           # bench.py --gpus N sets a dict here after its warm-up: see GradBucket.sync

    def __init__(self, generator, E, lpips_model, lr=0.0015, beta_1=0.0, batch_size=2, z_dim=512,
                 reference_noise=False, exact_ddp=True, mapping=None, stage=2, zero_grad_to_none=True):
        """`generator`, `mapping`: the models of one --mtype, see generators.make_adapter.
        `stage`: 2 = E_align_s2.py (image phase 1/5/9-weighted with gradient, then the latent phase); 1 = the stage-1 variant
        E_align_cropping_s1.py:185-218: the image-space losses are evaluated on detached inputs and summed unweighted (they are
        reported, not trained on: no gradient reaches E, the script's first optimizer step changes nothing) and only the
        latent phase updates the encoder.
        `zero_grad_to_none` (stage 1 only): True = `optimizer.zero_grad()` of torch >= 2.0 drops the gradients, so the script's
        first optimizer step finds none and changes nothing (tests/golden/step_s1.npz).  False = the torch < 2.0 default the
        reference's pinned environment has (python 3.7, torch 1.8 .. 1.13): gradients are zero-FILLED, so from the second
        iteration on that step runs LREQAdam with zero gradients - every step counter advances and every second moment decays
        by beta_2 (custom_adam.py:35-62), which makes the latent-phase updates ~1.4x larger in steady state
        (tests/golden/step_s1_legacy.npz).  Stage 2 is unaffected: both of its phases give every trained parameter a gradient."""
        self.zero_grad_to_none = bool(zero_grad_to_none)
        if stage not in (1, 2):
            raise ValueError("EAlignStep: stage must be 1 or 2")
        self.stage = stage
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        super().__init__(generator, E, lpips_model, mapping=mapping, lr=lr, beta_1=beta_1, batch_size=batch_size, z_dim=z_dim,
                         reference_noise=reference_noise)
        # DGE_FORCE_DIST=1 exercises the collective code path on a 1-rank group (single-GPU validation of the DDP wiring)
        self.dist_on = self.world > 1 or (os.environ.get("DGE_FORCE_DIST") == "1" and dist.is_initialized())
        self.exact_ddp = exact_ddp
        self.bucket = GradBucket(E, self.dev, exact_ddp) if self.dist_on else None       # the DDP gradient exchange
        if self.dist_on:
            E.__dict__["_early_grad_hook"] = self.bucket.early_reduce        # autograd_enc_bwd calls it after the deep blocks

    def _sync_grads(self):
        """data parallel: all-reduce of the encoder's gradients; returns the optimizer's grad_scale"""
        return None if self.bucket is None else self.bucket.sync(self.comm_stats)

    # ------------------------------------------------------------------ hipGraph replay of the iteration
    def capture(self, warmup=GraphReplay.WARMUP, start=0):
        """Captures one iteration into a hipGraph (single-GPU runs; the ≈1300 launches of a step cost ≈18 ms of host time,
        which bounds the step at the reference's default batch of 2).  Host-side decisions of an iteration become device
        inputs: z (static buffer), the style-mixing mask (StyleGAN2 train mode, same np.random draw order as the
        reference) and Adam's sqrt(1 - beta2^t) factors.  Encoder / StyleGAN1 noise comes from the project's counter-based
        generator, whose seed becomes a device scalar (ops.noise_graph_begin).  `warmup` real iterations run inside this call
        (plus one eager iteration in front of them in the legacy stage-1 form); the captured iteration itself is only recorded.
        The real iterations are numbered `start`, `start` + 1, ... (the number seeds z and the mixing mask,
        training_utils.py:46-52); `self.graph_iteration` is the number of the NEXT iteration when this returns - a training loop
        continues there (train() below) instead of repeating the warm-up's iterations."""
        if self.dist_on:
            raise RuntimeError("hipGraph capture is offered for single-process runs only (collectives are not captured)")
        # Capturing after EAGER steps of the same encoder used to end in a segmentation fault inside capture_end (round 2:
        # "crashed the runtime once"; reproduced with faulthandler in round 3).  Cause: the eager step's results (imgs2, w2) kept
        # their autograd graph alive, and with it the AccumulateGrad nodes of E's parameters, created on the default stream.
        # The captured iteration runs on a side stream; autograd re-uses the live nodes and inserts its cross-stream event
        # record / wait between the default stream and the capturing one - an illegal dependency for a capture.  step() now
        # returns detached results; dead graphs of earlier iterations are collected here before the warm-up, so that the
        # warm-up iterations create fresh accumulator nodes on the capture's side stream.
        import gc
        self.last = {}
        gc.collect()
        if not self.gen.capturable:
            raise RuntimeError("hipGraph capture is not offered for --mtype 4: z is a scipy truncnorm draw and the class id a host "
                               "decision of every iteration (E_align_s2.py:139-150); run the eager step")
        ops.noise_graph_begin(self.dev)          # noise kernels read their seed from a device scalar from here on
        self._g_z = torch.zeros(self.batch_size, self.z_dim, device=self.dev)
        self.gen.graph_inputs(self.dev)
        # optimizer calls of one iteration: two in stage 2 (image phase, latent phase), one in stage 1 - two again in its legacy
        # zero_grad form (tick() + step()), where the tick is skipped while no parameter has state yet: one eager iteration
        # first gives every parameter its state, so that every captured / replayed iteration makes the same number of calls
        calls = 2 if (self.stage == 2 or not self.zero_grad_to_none) else 1
        self.graph_iteration = int(start)
        if self.stage == 1 and not self.zero_grad_to_none and not any(len(st) for st in self.opt.state.values()):
            self.step(self.graph_iteration)
            self.graph_iteration += 1
        self.opt.graph_begin(calls, self.dev)
        return self._capture(lambda: self.step(0, z=self._g_z), warmup)

    def _graph_inputs(self, iteration):
        self._g_z.copy_(self._draw_z(iteration))
        self.gen.refresh_graph_inputs()
        self.opt.graph_advance()

    def replay(self, iteration=None):
        if iteration is not None:
            self.graph_iteration = iteration
        return super().replay()

    # ------------------------------------------------------------------ one iteration
    def _first_pass(self, iteration, z, gen_noise):
        """The head's generator pass, or the one the previous step prefetched (step() has checked that it is this iteration's)."""
        pref = self.__dict__.pop("_pref", None)
        if pref is not None:
            # the pass was issued on the side stream: the consumer orders itself behind the event recorded there (the issuing step's
            # own join at its end may not have run if that step raised in between)
            torch.cuda.current_stream(self.dev).wait_event(pref[4])
            z, imgs1, w1 = pref[1:4]
        else:
            z = self._z_on_device(iteration, z)
        # the re-pack of the encoder's conv weights (stale since the last optimizer step) beside the generator's first pass:
        # an HBM-bound copy next to small-grid low-resolution layers; joined in front of the encoder
        pack_side = None
        if (self.dev.type == "cuda" and _SIDE_STREAMS and _PACK_STREAM and not ops.is_deterministic() and pack_cache(self.E, create=False)
                and (self.batch_size * imgs_px(self.G) >= (4 << 20) or torch.cuda.is_current_stream_capturing())):
            if getattr(self, "_pack_stream", None) is None:
                self._pack_stream = torch.cuda.Stream(device=self.dev)
            pack_side, main = self._pack_stream, torch.cuda.current_stream(self.dev)
            pack_side.wait_stream(main)
            with torch.cuda.stream(pack_side):
                refresh_packs(self.E)
        if pref is None:
            with torch.no_grad():
                imgs1, w1 = self.gen.sample(z, gen_noise)
        if pack_side is not None:
            torch.cuda.current_stream(self.dev).wait_stream(pack_side)
        return z, imgs1, w1

    def cancel_prefetch(self):
        """Drops a generator pass that step(..., prefetch_next=True) issued for an iteration that will not run (end of a loop that
        could not know it was at its end).  The generator's own state has seen that pass (StyleGAN2 train mode: one w_avg update) and
        so have the random generators; returns the iteration number it belonged to, or None."""
        pref = self.__dict__.pop("_pref", None)
        return None if pref is None else pref[0]

    def _prefetch_ok(self):
        # (data parallel: the prefetched pass's only collective is the w_avg mean - 512 floats behind the mapping network, the first
        #  ~0.1 ms of the pass - issued from the side stream in the same program order on every rank.  ProcessGroupNCCL runs a group's
        #  collectives in call order on its own stream, so this one sits in front of the iteration's loss sums and gradient buckets and is
        #  long done when they are issued, several ms later: no exposed serialisation is expected.  Measured only with a one-rank RCCL
        #  group and two gloo ranks (tests/test_ddp_gpu.py); `--no-prefetch` / prefetch_next=False is the serial form.)
        return (_SIDE_STREAMS and self.stage == 2 and self.dev.type == "cuda" and self.gen.prefetchable and not self.reference_noise
                and not ops.is_deterministic() and not torch.cuda.is_current_stream_capturing())

    def step(self, iteration, z=None, noises=None, gen_noises=(None, None), new_z=None, prefetch_next=False):
        """`noises`: optional encoder noise tensors; `gen_noises`: optional (first, second) generator noise lists for
        generators that draw noise per call (StyleGAN1); `new_z`: the style-mixing latent of StyleGAN2's train mode -- all only
        for parity runs against captured reference noise.
        `prefetch_next`: the caller's promise that its next call is step(iteration + 1) with default inputs (a training loop).  The
        generator pass that opens that iteration - set_seed(iteration + 1), z, G(z) under no_grad: the training DATA of the encoder, which
        depends on nothing the encoder does (E_align_s2.py:102-115) - is then issued on a side stream beside this iteration's image
        losses and backward passes, whose low-resolution launches leave most of the chip idle (measured at batch 8, same box: 22.07 ->
        21.56 ms per step).  Same work per iteration, same numbers: nothing between that point (behind E(imgs1) and synthesis(w2), the
        last consumers of random numbers and of the generator's state in an iteration) and the next iteration's start draws a random
        number or reads w_avg, so every draw and the w_avg update happen in the order of the serial loop.  A step that finds a
        prefetched pass it was not promised (another iteration number, explicit inputs) raises instead of silently using or dropping it."""
        # the promise is checked before this call has any side effect: a mismatch leaves the prefetched pass where it is
        # (cancel_prefetch() drops it) and the step object as it was
        pref = self.__dict__.get("_pref")
        if pref is not None and (pref[0] != iteration or z is not None or noises is not None or new_z is not None or gen_noises != (None, None)):
            raise RuntimeError(f"step({iteration}): the previous step prefetched the generator pass of iteration {pref[0]} with default "
                               "inputs (prefetch_next=True is a promise about the next call)")
        z, imgs1, w1, const2, w2, imgs2 = self._head(iteration, z, noises, gen_noises, new_z)

        gctx = losses.GlobalBatch(self.world) if (self.dist_on and self.exact_ddp) else None
        pf_side = None

        def issue_prefetch():
            # the next iteration's generator pass on a side stream (see the docstring).  The side stream starts behind everything
            # queued so far; its results are handed to the next call after the join at the end of this one.
            nonlocal pf_side
            if getattr(self, "_pf_stream", None) is None:
                self._pf_stream = torch.cuda.Stream(device=self.dev)
            pf_side, main = self._pf_stream, torch.cuda.current_stream(self.dev)
            pf_side.wait_stream(main)
            with torch.cuda.stream(pf_side):
                nxt = TrainStep._first_pass(self, iteration + 1, None, None)      # the plain head with default inputs
                done = torch.cuda.Event()
                done.record(pf_side)
            for t in nxt:
                t.record_stream(main)
            self._pref = (iteration + 1,) + tuple(nxt) + (done,)
        # (a parity run that injects its own style-mixing latent leaves it on the adapter: the next iteration's pass must not see it)
        do_pf = prefetch_next and self._prefetch_ok() and self.gen.new_z is None
        if do_pf and _PREFETCH_AT == "loss":
            issue_prefetch()
        if self.stage == 1:
            # E_align_cropping_s1.py:185-203: .detach().clone() on every loss input, loss_tsa = imgs + medium + small
            with torch.no_grad():
                loss_tsa, info_img = losses.image_loss_tsa(imgs1, imgs2.detach(), self.lpips, weights=(1.0, 1.0, 1.0), global_batch=gctx)
            if not self.zero_grad_to_none:
                self.opt.tick()          # E_align_cropping_s1.py:203-205 under torch < 2.0: optimizer step on zero-filled gradients
        else:
            loss_tsa, info_img = losses.image_loss_tsa(imgs1, imgs2, self.lpips, global_batch=gctx)
            self.opt.zero_grad()
            if do_pf and _PREFETCH_AT == "bwd1":
                issue_prefetch()
            loss_tsa.backward(retain_graph=True)
            gs = self._sync_grads()
            self.opt.step(grad_scale=gs)

        loss_w, info_w = losses.space_loss(w1, w2, image_space=False, global_batch=gctx)
        loss_mtv = loss_w * 0.01
        self.opt.zero_grad()
        if do_pf and pf_side is None:
            issue_prefetch()
        loss_mtv.backward()
        gs = self._sync_grads()
        self.opt.step(grad_scale=gs)
        if pf_side is not None:
            torch.cuda.current_stream(self.dev).wait_stream(pf_side)
        ops.zero_arena_end()
        det = self.det
        self.last = dict(imgs1=imgs1, imgs2=det(imgs2), w1=det(w1), w2=det(w2), const2=det(const2), loss_tsa=loss_tsa.detach(),
                         info_img=info_img, loss_w=loss_w.detach(), info_w=info_w)
        return self.last


_SIDE_STREAMS = os.environ.get("DGE_SIDE_STREAMS", "1") != "0"
# where step(prefetch_next=True) issues the next iteration's generator pass: beside the image losses ("loss"), the first backward
# ("bwd1") or the second backward ("bwd2").  Same box, batch 8, two rounds: serial 22.07 / 22.23 ms, bwd2 21.70 / 21.81, bwd1 21.71 / 21.78, loss 21.56 / 21.67
_PREFETCH_AT = os.environ.get("DGE_PREFETCH_AT", "loss")
# the early weight re-pack beside the generator's first pass: - 0.13 ms in round 3, + 0.08 ms against this round's kernels (three
# same-box pairs, 24.08 vs 24.17 ms): opt-in
_PACK_STREAM = os.environ.get("DGE_PACK_STREAM", "0") == "1"


def train(tensor_writer=None, args=None):
    """Reference E_align_s2.train() (flags: E_align_s2.py:304-318)."""
    G, Gm, E, LP = load_models(args)
    prepare_training(args, LP)
    st = EAlignStep(G, E, LP, lr=args.lr, beta_1=args.beta_1, batch_size=args.batch_size, z_dim=args.z_dim, mapping=Gm,
                    stage=getattr(args, "stage", 2), zero_grad_to_none=not getattr(args, "legacy_zero_grad", False))
    # Launch mode.  At the reference's default batch (2, E_align_s2.py:308) the eager step is bound by the host's launch rate
    # (~560 launches): single-process runs at batch <= 2 therefore replay the iteration from a captured hipGraph by default
    # (EAlignStep.capture: z, style-mixing mask and Adam factors become device inputs; same numbers, see
    # tests/test_step_gpu.py::test_graph_replay_*).  --launch eager / graph overrides; --mtype 4 and the deterministic mode stay eager.
    mode = getattr(args, "launch", "auto")
    use_graph = mode == "graph" or (mode == "auto" and not st.dist_on and args.batch_size <= 2 and args.mtype != 4
                                    and not getattr(args, "deterministic", False))
    first = 0
    prefetch = not getattr(args, "no_prefetch", False)
    # what runs for real before the first replay: iteration 0 eagerly (below), capture()'s warm-up iterations and one more eager
    # iteration in the legacy stage-1 form: a run no longer than that stays eager
    if use_graph and args.iterations <= 1 + GraphReplay.WARMUP + 1:
        use_graph = False
    if use_graph:
        # iteration 0 runs eagerly: the reference logs its losses and dumps E_model_ep0_iter0.pth right after it
        # (E_align_s2.py: iteration % 100 == 0, iteration % 5000 == 0) - the dump holds the encoder after ONE iteration, as its name says
        r = st.step(0)
        print("ep_0_iter_0", "loss_tsa", float(r["loss_tsa"]), "loss_w", float(r["loss_w"]))
        if getattr(args, "experiment_dir", None):
            torch.save(E.state_dict(), "%s/E_model_ep0_iter0.pth" % args.experiment_dir)
        st.capture(start=1)
        first = st.graph_iteration   # capture() ran iterations 1 .. first - 1 for real (its warm-up): the loop continues behind them,
        # so that `--launch graph` and `--launch eager` make the same number of encoder updates on the same z / mask sequence
        print("ep_0_iter_1 .. %d ran inside the graph capture (warm-up)" % (first - 1))
    for iteration in range(first, args.iterations):
        # (eager launches: the next iteration's generator pass goes out beside this iteration's second backward, EAlignStep.step)
        r = st.replay(iteration) if use_graph else st.step(iteration, prefetch_next=(prefetch and iteration + 1 < args.iterations))
        if iteration % 100 == 0:
            print("ep_%d_iter_%d" % (iteration // 30000, iteration % 30000), "loss_tsa", float(r["loss_tsa"]),
                  "loss_w", float(r["loss_w"]))
        if iteration % 5000 == 0 and getattr(args, "experiment_dir", None):
            torch.save(E.state_dict(), "%s/E_model_ep%d_iter%d.pth" % (args.experiment_dir, iteration // 30000, iteration % 30000))
    return st


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="the training args")
    add_train_args(parser, iterations=210000)
    add_model_args(parser)
    parser.add_argument("--launch", choices=("auto", "eager", "graph"), default="auto",
                        help="auto: hipGraph replay of the iteration for single-process runs at batch <= 2, eager otherwise")
    parser.add_argument("--no_prefetch", action="store_true", help="eager launches: run the generator pass of iteration n + 1 at the start of that "
                        "iteration instead of beside the second backward of iteration n (same numbers either way)")
    parser.add_argument("--stage", type=int, default=2, help="2: E_align_s2.py; 1: E_align_cropping_s1.py (latent phase only trains E)")
    parser.add_argument("--legacy_zero_grad", action="store_true", help="stage 1: optimizer.zero_grad() as torch < 2.0 (zero-filled gradients, the "
                        "reference's pinned environment): the first optimizer step of an iteration ticks every Adam state")
    return parser


def main(argv=None):
    return train(None, build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
