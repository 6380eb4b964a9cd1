"""Derived copies of a weight (packed bf16, MFMA-fragment order, data-gradient transposes, conv_pp weight images, dense forms,
sum-of-squares tables), each valid until the parameter is written.

Two things write a parameter: torch in-place ops, which bump `Tensor._version`, and this package's own kernels
(dge_lreq_adam_multi, like the reference's `p.data` update), which write through the raw pointer and bump nothing.  For the
second kind the parameter carries a generation counter, `_dge_gen`, that only this module reads or writes: whoever writes
parameters behind torch's back calls `written(params)` afterwards.  "Is my copy still valid" is `version(w)`; what tells two
copies of one weight apart (pack mode, dtype, "pp", ...) belongs in the cache KEY, never in the version.

Plain caches (one dict per module, `lookup` / `store`): each copy is rebuilt on its own at its first stale use.
Grouped cache of the encoder family (`pack_cache`, `packed`, `refresh_packs`, `prime_pack_tables`): an optimizer step makes
every copy of the module stale at once, and one launch refreshes them all."""
from . import ops


def version(w):
    return (w._version, w.data_ptr(), getattr(w, "_dge_gen", 0))


def written(params):
    """The caller has written these parameters through the raw pointer (or re-loaded them): every derived copy is stale.
    Host-side bookkeeping only: inside a hipGraph capture it runs once, at capture, and no replay depends on it."""
    for p in params:
        p._dge_gen = getattr(p, "_dge_gen", 0) + 1


def save(params):
    """-> token for `restore`: around a write that provably changes no value (LREQAdam.tick), so that every copy stays valid"""
    return [(p, getattr(p, "_dge_gen", 0)) for p in params]


def restore(token):
    for p, gen in token:
        p._dge_gen = gen


def lookup(cache, key, w):
    """The copy of `w` stored under `key`, or None when there is none or `w` was written since (then build it and `store` it)."""
    hit = cache.get(key)
    if hit is not None and hit[0] == (w._version, w.data_ptr(), getattr(w, "_dge_gen", 0)):
        return hit[1]
    return None


def store(cache, key, w, copy):
    cache[key] = (version(w), copy)
    return copy


# ------------------------------------------------------------------ grouped cache of the encoder family
# entry: cache[(id(w), mode, dtype)] = [version, packed copy, w]; the reference to w keeps id(w) from being reused by another
# parameter while the entry lives.  cache[("_pack_scratch", kind of refresh)]: descriptor table of pack_conv_weights_multi.
def pack_cache(module, create=True):
    """The module's grouped cache (None when `create` is false and no copy was ever made)."""
    if create:
        return module.__dict__.setdefault("_pack_cache", {})
    return module.__dict__.get("_pack_cache")


def _is_bwd_mode(mode):
    return (mode & 0xff) in (ops.PACK_DGRAD, ops.PACK_UPFOLD_DGRAD, ops.PACK_SG1_UP_DGRAD, ops.PACK_UPT2D_DGRAD)


def _stale(cache, only_bwd=False):
    return [(k, e) for k, e in cache.items() if isinstance(k, tuple) and len(k) == 3 and isinstance(e, list) and version(e[2]) != e[0]
            and (not only_bwd or _is_bwd_mode(k[1]))]


def _refresh(cache, stale, which):
    """One launch for all of `stale`; a descriptor table (device scratch) per kind of refresh, so that the two alternating sets of
    a step (everything / data-gradient copies only) each find their table already uploaded (a hipGraph capture cannot upload)."""
    key = ("_pack_scratch", which)
    cache[key] = ops.pack_conv_weights_multi([(e[2].detach(), k[1], k[2], 1.0, e[1]) for k, e in stale], cache.get(key))
    for k, e in stale:
        e[0] = version(e[2])


def refresh_packs(module):
    """Refreshes every stale packed copy of the module's conv weights now (on the current stream): EAlignStep runs this beside the
    generator's first pass at the start of an iteration instead of in front of the encoder's first conv."""
    cache = pack_cache(module, create=False)
    if cache:
        stale = _stale(cache)
        if stale:
            _refresh(cache, stale, "all")


def prime_pack_tables(module):
    """EAlignStep.capture, between the eager warm-up and the capture: uploads the descriptor table of the all-copies refresh (a
    capture cannot upload; a single warm-up iteration has only used the data-gradient table) and leaves every copy marked stale,
    so that the captured iteration re-packs exactly as a steady-state iteration does."""
    cache = pack_cache(module, create=False)
    if cache:
        stale = _stale(cache)
        if stale:
            _refresh(cache, stale, "all")
            for _, e in stale:
                e[0] = None


def packed(cache, conv, dtype, mode, hw=None):
    """Packed copy of a conv weight, rebuilt when the parameter was updated in place.  An optimizer step makes EVERY copy of
    the module stale at once: the first stale hit of a FORWARD copy refreshes all of them in one launch
    (ops.pack_conv_weights_multi) - in place, the consumers of the old values are earlier on the same stream; the first stale
    hit of a data-gradient copy (the second backward of an E_align step, after the first optimizer step) refreshes the
    data-gradient copies only - the forward copies would be stale again before their next use.  `hw`: resolution the conv runs
    at (the low-resolution blocks keep their copies in fragment order for csrc/conv_small.hip)."""
    w = conv.weight
    if hw is not None:
        mode = ops.pack_mode_for(w, mode, hw, hw, dtype)
    key = (id(w), mode, dtype)
    ver = version(w)
    hit = cache.get(key)
    if hit is not None and hit[0] == ver:
        return hit[1]
    if hit is None:
        cache[key] = [ver, ops.pack_conv_weight(w, mode, dtype, 1.0), w]
        return cache[key][1]
    bwd = _is_bwd_mode(mode)
    _refresh(cache, _stale(cache, only_bwd=bwd), "bwd" if bwd else "all")
    return cache[key][1]
