"""weight_cache: "derived copy of a weight, valid until the parameter is written" - on CPU tensors, with counting stand-ins for
the builders (the pack kernels themselves are covered by the GPU suites)."""
import torch
from torch import nn

from dge_amd import ops, weight_cache as wc


class Builder:
    """Counting stand-in for a pack launch: the copy is a clone, so a stale copy is visible as a wrong value."""

    def __init__(self):
        self.builds = 0

    def __call__(self, w):
        self.builds += 1
        return w.detach().clone()


def cached(cache, key, w, build):
    hit = wc.lookup(cache, key, w)
    return hit if hit is not None else wc.store(cache, key, w, build(w))


def test_version_changes_on_every_kind_of_write():
    w = nn.Parameter(torch.randn(4, 3))
    v0 = wc.version(w)
    assert wc.version(w) == v0
    with torch.no_grad():
        w.add_(1.0)                                   # torch in-place op
    v1 = wc.version(w)
    assert v1 != v0
    wc.written([w])                                   # raw-pointer write (LREQAdam.step, begin_image)
    v2 = wc.version(w)
    assert v2 != v1 and v2 != v0
    w.data = torch.randn(4, 3)                        # storage replaced
    assert wc.version(w) not in (v0, v1, v2)


def test_unchanged_parameter_is_served_without_a_build():
    w, cache, build = nn.Parameter(torch.randn(4, 3)), {}, Builder()
    first = cached(cache, "w", w, build)
    assert build.builds == 1
    for _ in range(5):
        assert cached(cache, "w", w, build) is first
    assert build.builds == 1


def test_each_kind_of_write_rebuilds_once():
    w, cache, build = nn.Parameter(torch.randn(4, 3)), {}, Builder()
    cached(cache, "w", w, build)
    with torch.no_grad():
        w.mul_(2.0)
    assert torch.equal(cached(cache, "w", w, build), w) and build.builds == 2
    w.data.view(-1)[0] = 7.0                          # what a kernel does through the raw pointer: no version bump ...
    wc.written([w])                                   # ... hence the notification
    assert torch.equal(cached(cache, "w", w, build), w) and build.builds == 3
    w.data = torch.randn(4, 3)
    assert torch.equal(cached(cache, "w", w, build), w) and build.builds == 4
    cached(cache, "w", w, build)
    assert build.builds == 4


def test_tick_sequence_keeps_every_copy_valid():
    """save -> written -> restore: LREQAdam.tick (a step that changes no value) leaves the cached copies valid."""
    ws = [nn.Parameter(torch.randn(4, 3)) for _ in range(3)]
    wc.written(ws[:1])                                # the counters need not start equal
    cache, build = {}, Builder()
    first = [cached(cache, i, w, build) for i, w in enumerate(ws)]
    token = wc.save(ws)
    wc.written(ws)
    wc.restore(token)
    assert all(cached(cache, i, w, build) is c for (i, w), c in zip(enumerate(ws), first))
    assert build.builds == 3


def test_two_keys_on_one_weight_coexist_and_go_stale_together():
    w, cache, build = nn.Parameter(torch.randn(4, 3)), {}, Builder()
    keys = [("w", ops.BF16), ("w", ops.F32), ("dg", ops.BF16, ops.PACK_DGRAD)]
    first = [cached(cache, k, w, build) for k in keys]
    assert build.builds == 3
    assert all(cached(cache, k, w, build) is c for k, c in zip(keys, first))      # alternating keys does not evict
    assert build.builds == 3
    wc.written([w])
    again = [cached(cache, k, w, build) for k in keys]
    assert build.builds == 6 and all(a is not c for a, c in zip(again, first))


# ------------------------------------------------------------------ grouped cache of the encoder family
class Packs:
    """Stand-ins for ops.pack_conv_weight / ops.pack_conv_weights_multi that count launches and record what each refreshed."""

    def __init__(self, monkeypatch):
        self.single, self.multi = 0, []
        monkeypatch.setattr(ops, "pack_conv_weight", self.pack)
        monkeypatch.setattr(ops, "pack_conv_weights_multi", self.pack_multi)

    def pack(self, w, mode, dtype, scale):
        self.single += 1
        return w.detach().clone()

    def pack_multi(self, entries, scratch=None):
        self.multi.append(sorted(mode for _, mode, _, _, _ in entries))
        for w, _, _, _, out in entries:
            out.copy_(w)                              # in place, like the kernel
        return scratch or ["table"]


def _enc():
    E = nn.Module()
    E.conv_1, E.conv_2 = nn.Conv2d(3, 4, 3, bias=False), nn.Conv2d(4, 4, 3, bias=False)
    return E


def _all_packs(E):
    cache = wc.pack_cache(E)
    return [wc.packed(cache, conv, ops.BF16, mode) for conv in (E.conv_1, E.conv_2) for mode in (ops.PACK_FWD, ops.PACK_DGRAD)]


def test_pack_cache_accessor():
    E = _enc()
    assert wc.pack_cache(E, create=False) is None
    wc.refresh_packs(E); wc.prime_pack_tables(E)      # nothing cached: nothing to do
    cache = wc.pack_cache(E)
    assert cache == {} and wc.pack_cache(E) is cache and wc.pack_cache(E, create=False) is cache


def test_grouped_refresh_rules(monkeypatch):
    packs, E = Packs(monkeypatch), _enc()
    cache = wc.pack_cache(E)
    first = _all_packs(E)
    assert packs.single == 4 and packs.multi == []
    assert all(a is b for a, b in zip(_all_packs(E), first)) and packs.single == 4 and packs.multi == []
    params = [E.conv_1.weight, E.conv_2.weight]
    fwd2, bwd2 = [ops.PACK_FWD] * 2, [ops.PACK_DGRAD] * 2

    def write():
        for p in params:
            p.data.add_(1.0)
        wc.written(params)
    # first stale hit of a forward copy: ALL copies in one launch, in place
    write()
    assert wc.packed(cache, E.conv_1, ops.BF16, ops.PACK_FWD) is first[0]
    assert packs.multi == [sorted(fwd2 + bwd2)]
    assert all(a is b for a, b in zip(_all_packs(E), first)) and len(packs.multi) == 1 and packs.single == 4
    assert torch.equal(first[3], E.conv_2.weight)
    # first stale hit of a data-gradient copy: the data-gradient copies only; the forward ones follow at their own first use
    write()
    assert wc.packed(cache, E.conv_2, ops.BF16, ops.PACK_DGRAD) is first[3]
    assert packs.multi[1:] == [bwd2]
    assert torch.equal(first[1], E.conv_1.weight) and not torch.equal(first[0], E.conv_1.weight)
    _all_packs(E)
    assert packs.multi[1:] == [bwd2, fwd2]
    assert torch.equal(first[0], E.conv_1.weight)
    # one descriptor table per kind of refresh
    assert {k[1] for k in cache if k[0] == "_pack_scratch"} == {"all", "bwd"}
    # refresh_packs: everything stale, now, in one launch; then nothing left to do
    write()
    n = len(packs.multi)
    wc.refresh_packs(E)
    assert packs.multi[n:] == [sorted(fwd2 + bwd2)]
    wc.refresh_packs(E); _all_packs(E)
    assert len(packs.multi) == n + 1
    # the tick sequence leaves the grouped copies valid too
    token = wc.save(params)
    wc.written(params)
    wc.restore(token)
    _all_packs(E)
    assert len(packs.multi) == n + 1 and packs.single == 4


def test_prime_pack_tables_leaves_every_copy_stale(monkeypatch):
    packs, E = Packs(monkeypatch), _enc()
    cache = wc.pack_cache(E)
    first = _all_packs(E)
    wc.prime_pack_tables(E)                           # nothing stale: nothing uploaded, nothing marked
    assert packs.multi == []
    wc.written([E.conv_1.weight, E.conv_2.weight])
    wc.prime_pack_tables(E)
    assert len(packs.multi) == 1 and len(packs.multi[0]) == 4 and ("_pack_scratch", "all") in cache
    assert wc.packed(cache, E.conv_1, ops.BF16, ops.PACK_FWD) is first[0]         # the captured iteration re-packs everything
    assert len(packs.multi) == 2 and len(packs.multi[1]) == 4
    _all_packs(E)
    assert len(packs.multi) == 2 and packs.single == 4


def test_entry_of_a_replaced_parameter_is_not_served_for_its_replacement(monkeypatch):
    """The grouped cache keys on id(w): safe only while each entry keeps its parameter alive (an id is reused after a free)."""
    Packs(monkeypatch)
    E = _enc()
    cache = wc.pack_cache(E)
    for _ in range(50):
        old = E.conv_1.weight
        old_copy = wc.packed(cache, E.conv_1, ops.BF16, ops.PACK_FWD)
        assert any(e[2] is old for k, e in cache.items() if k[0] == id(old))      # the entry holds the parameter
        E.conv_1.weight = nn.Parameter(torch.randn_like(old))
        del old                                       # without that reference the allocator could hand the same id out again
        new_copy = wc.packed(cache, E.conv_1, ops.BF16, ops.PACK_FWD)
        assert new_copy is not old_copy and torch.equal(new_copy, E.conv_1.weight)
