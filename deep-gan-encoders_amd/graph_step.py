"""hipGraph capture and replay of one training iteration, written once for every step class that offers it (EAlignStep, EmbedStep,
LatentEmbedStep and the other TwoPhaseEmbedStep subclasses, ProjectorStep).  At small batches an eager iteration is bound by the
host's launch rate (500 - 1700 launches, all on the current stream through the C ABI); the captured iteration re-runs with one graph
launch.

The step class provides its optimisers, `_graph_opts()` -> [(optimiser, step() calls per iteration)] (default: `opt` alone, on which
the class has called graph_begin itself; LREQAdam and Adam offer the same graph_* interface), optionally an encoder `E` whose pack
tables are primed before the capture, and `_graph_inputs(iteration)`: the upload of everything the host decides per iteration into
the device buffers the iteration reads - Adam's step factors (`graph_advance()` of every optimiser) and the class's own (z, mixing
mask, noise seed).  Their order is the class's and shows in the time of a replay: the host does not run ahead of the device here
(100 replay() calls return in the time 99 replays take), so host work that moves behind the first upload is exposed (EmbedStep at
1024^2: 12.57 -> 12.72 ms per replay with the noise seed uploaded in front of graph_advance instead of behind it, four alternating
pairs)."""
import collections

import torch


class GraphReplay:
    WARMUP = 2                  # real iterations capture() runs by default before it records one
    graph_iteration = 0         # number of the NEXT iteration to execute; seeds its host-side inputs
    _graph = None

    @property
    def captured(self):
        """True once an iteration has been captured: replay() and the static inputs are available."""
        return self._graph is not None

    def _graph_opts(self):
        """[(optimiser, step() calls per iteration)] of the iteration; None: the class calls graph_begin itself."""
        return [(self.opt, None)]

    def _capture(self, run, warmup, after_warmup=None):
        """Runs `warmup` real iterations `run()`, then RECORDS one more into a hipGraph and returns its static result dict.
        `after_warmup()` runs behind the last real iteration, on its stream.  The host counters of every optimiser of _graph_opts()
        are snapshotted at ONE point, behind the last real iteration and before _graph_inputs of the recorded one (LatentEmbedStep
        used to snapshot its second optimiser in after_warmup: that is behind the last real iteration and before the recorded
        one's _graph_inputs too, and nothing in between touches an optimiser, so the values are the same)."""
        # the warm-up runs on a side stream, like the capture behind it and never on the default stream (what autograd binds to
        # the stream of an iteration must not tie the capture to the default stream: see the comment in EAlignStep.capture),
        # joined with the current stream on both ends
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._graph_inputs(self.graph_iteration)
                self.graph_iteration += 1
                run()
            if after_warmup is not None:
                after_warmup()
        torch.cuda.current_stream().wait_stream(side)
        E = getattr(self, "E", None)
        if E is not None:
            from .weight_cache import prime_pack_tables
            prime_pack_tables(E)            # (the all-copies descriptor table must be on the device before the capture)
        graph = torch.cuda.CUDAGraph()
        # the captured iteration is RECORDED, not executed: `graph_iteration` does not move and the counters its step() calls
        # advance on the host (Adam's t) are rolled back, so that the first replay is the iteration behind the warm-up's last
        snaps = [(opt, opt.graph_snapshot()) for opt, _ in self._graph_opts()]
        self._graph_inputs(self.graph_iteration)
        with torch.cuda.graph(graph):
            self._g_out = run()
        for opt, snap in snaps:
            opt.graph_restore(snap)
        self._graph = graph
        return self._g_out

    def _capture_keeping_last(self, run, warmup, after_warmup=None):
        """_capture for a step that keeps its latest results in `self.last`: behind it `self.last` holds those of the last EXECUTED
        iteration (tensors cloned; {} without a warm-up), not those of the recorded one.  `after_warmup()` runs in front of the clone."""
        warm = {}

        def keep_last():
            if after_warmup is not None:
                after_warmup()
            if warmup:
                warm.update({k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.last.items()})
        out = self._capture(run, warmup, after_warmup=keep_last)
        self.last = warm
        return out

    def replay(self):
        """Executes iteration `graph_iteration` with one graph launch; returns the static result dict."""
        self._graph_inputs(self.graph_iteration)
        self.graph_iteration += 1
        self._graph.replay()
        for opt, _ in self._graph_opts():
            opt.graph_count_replay()
        return self._g_out

    def _set_static(self, name, t):
        """Copies `t` into the static input `name` that the captured iteration reads on every replay."""
        who = type(self).__name__
        if not self.captured:
            raise RuntimeError(f"{who}: no captured iteration (call capture() first)")
        buf = getattr(self, name)
        if tuple(t.shape) != tuple(buf.shape) or t.dtype != buf.dtype or t.device != buf.device:
            raise ValueError(f"{who}: the captured iteration works on {tuple(buf.shape)} {buf.dtype} on {buf.device}, got "
                             f"{tuple(t.shape)} {t.dtype} on {t.device}; re-capture for a new geometry")
        buf.copy_(t.detach())

    def _reset_opt(self):
        """Fresh optimizer state for a new image group."""
        if getattr(self.opt, "_graph_corr", None) is not None:
            self.opt.graph_reset()          # same device addresses: a captured graph stays valid
        else:
            self.opt.state = collections.defaultdict(dict)
