"""Collectives of the data-parallel runs (one process per GPU): the all-reduce every module uses (RCCL, or gloo staged through
the host) and the flat gradient bucket of the encoder.  Nothing here knows a training step; the loss (losses.GlobalBatch), the
StyleGAN2 generator (w_avg) and the steps import from here."""
import torch
import torch.distributed as dist


class _StagedWork:
    """all-reduce of a device tensor through a host copy (gloo builds without device support): wait() writes the result back"""

    def __init__(self, t, host, work):
        self.t, self.host, self.work = t, host, work

    def wait(self):
        if self.work is not None:
            self.work.wait()
        self.t.copy_(self.host)


def all_reduce(t, async_op=False):
    """Sum over ranks, in place.  RCCL ("nccl") reduces device tensors directly; with the gloo backend (the 2-process parity
    test on one GPU, CPU-only debugging) device tensors are staged through the host."""
    if t.is_cuda and dist.get_backend() == "gloo":
        host = t.detach().cpu()
        work = dist.all_reduce(host, op=dist.ReduceOp.SUM, async_op=async_op)
        st = _StagedWork(t, host, work if async_op else None)
        if async_op:
            return st
        st.wait()
        return None
    return dist.all_reduce(t, op=dist.ReduceOp.SUM, async_op=async_op)


class GradBucket:
    """One flat f32 bucket for all gradients of `module` (the encoder), exchanged once per phase: `early_reduce` from inside the
    backward for the gradients that exist early, `sync` for the rest.  `exact`: every rank differentiated the GLOBAL loss w.r.t.
    its own samples, the exchange is a sum; otherwise the losses are local and `sync` returns the 1/world scale of a mean."""

    def __init__(self, module, device, exact):
        self.module, self.dev, self.exact = module, device, exact
        self.world = dist.get_world_size()
        self._flat = self._layout = self._early_work = None

    def _views(self, early_names=()):
        """The layout: the parameters named in `early_names` first (their gradients exist long before the backward ends), the rest after."""
        lay = self._layout
        if lay is None or lay["early"] != tuple(early_names):
            named = dict(self.module.named_parameters())
            order = [n for n in early_names if n in named] + [n for n in named if n not in set(early_names)]
            n_early = sum(named[n].numel() for n in early_names if n in named)
            total = sum(p.numel() for p in named.values())
            self._flat = torch.empty(total, dtype=torch.float32, device=self.dev)
            views, off = {}, 0
            for n in order:
                views[n] = self._flat[off:off + named[n].numel()].view_as(named[n])
                off += named[n].numel()
            lay = self._layout = dict(early=tuple(early_names), views=views, n_early=n_early, named=named)
        return lay

    def early_reduce(self, grads):
        """Called from inside the encoder backward as soon as the gradients of the deep (512-channel) blocks exist: > 90 % of
        the 97 MB bucket.  Their all-reduce is issued asynchronously (RCCL's own stream) and runs under the backward of the
        high-resolution blocks, which is most of the backward's time; `sync` exchanges the remainder and joins."""
        if not grads:
            return
        lay = self._views(tuple(grads.keys()))
        names = [n for n in lay["early"] if grads.get(n) is not None]
        if len(names) != len(lay["early"]):
            return                                          # a different set than the layout was built for: leave it to sync
        torch._foreach_copy_([lay["views"][n] for n in names], [grads[n] for n in names])
        # Stream order: the copies above are queued on the CURRENT (compute) stream; ProcessGroupNCCL enqueues every collective on
        # its own stream behind an event it records on the current stream at call time (ProcessGroupNCCL::collective ->
        # syncStream), so the all-reduce reads the bucket after the copies without an explicit wait_stream here.  The rest of
        # the backward never touches [0, n_early) of the bucket (disjoint views), the bucket itself is owned by `self` (no
        # allocator reuse while the collective runs), and `_sync_grads` joins with work.wait(), which makes the compute stream wait
        # for RCCL's before the optimizer reads the sums.
        self._early_work = all_reduce(self._flat[:lay["n_early"]], async_op=True)

    def sync(self, comm_stats=None):
        """All-reduce (sum) of every gradient through the flat bucket; p.grad become views of it.  Returns the optimizer's grad_scale.
        `comm_stats` (bench.py --gpus N): a dict that collects events on the compute stream around the part of the exchange the step
        waits for - the remainder bucket plus whatever of the early bucket the backward did not cover - and both parts' byte counts."""
        work, self._early_work = self._early_work, None
        lay = self._views(self._layout["early"] if self._layout is not None else ())
        early, n_early = (set(lay["early"]), lay["n_early"]) if work is not None else (set(), 0)
        rest = [(n, p) for n, p in lay["named"].items() if p.grad is not None and n not in early]
        # one multi-tensor copy instead of ~100 small ones (they sit on the critical path in front of the collective)
        if rest:
            torch._foreach_copy_([lay["views"][n] for n, _ in rest], [p.grad for _, p in rest])
        for n, p in lay["named"].items():
            if p.grad is None and n not in early:           # parameters without a gradient this phase contribute zeros
                lay["views"][n].zero_()
        if comm_stats is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        all_reduce(self._flat[n_early:])
        if work is not None:
            work.wait()
        if comm_stats is not None:
            e1.record()
            comm_stats["events"].append((e0, e1))
            comm_stats["early_bytes"], comm_stats["remainder_bytes"] = 4 * n_early, 4 * (self._flat.numel() - n_early)
        for n, p in lay["named"].items():
            if p.grad is not None:
                p.grad = lay["views"][n]
        return None if self.exact else torch.full((1,), 1.0 / self.world, device=self.dev)
