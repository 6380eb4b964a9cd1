"""What the hand-written encoder walks share (E.BE: autograd_enc / autograd_enc_bwd; E_Blur, E_Blur_Z, E_Blur_W, E_Blur_W_2:
autograd_encblur; E_PG: autograd_encpg; E_BIG: autograd_encbig): the tails every backward ends with, the table of the grouped
`inver_mod` heads with its forward and backward, the block iterator, and the layer steps.  A step launches what its call sites
launched one by one, in that order; the statistics container is the caller's (ops.SlotStats in E.BE, ops.zeros((B, C, 2)) elsewhere)."""
import numpy as np
import torch

from . import ops
from .weight_cache import packed


def draw_noises(E, B, R, device):
    """The encoder's per-layer noise tensors ([B,1,r,r], two per block, one for the last): one generator launch for all of
    them, handed out as contiguous slices (the reference draws 17 separate CPU tensors, model/E/E.py:60,73 - quirk Q6).  Under
    data parallelism each tensor is the rank's slice of the draw a single process would make for the global batch."""
    shapes = []
    for j in range(E.layer_count):
        r = R >> j
        shapes.append((B, 1, r, r))
        if j != E.layer_count - 1:
            shapes.append((B, 1, r, r))
    if torch.device(device).type == "cpu":        # reference_noise mode: the reference's own sequence of CPU draws
        return [torch.randn(*s) for s in shapes]
    return ops.randn_rows(shapes, device)       # counter-based: the rank's rows of the global-batch draw (csrc/rng_kernels.hip)


# ------------------------------------------------------------------ tails shared by the hand-written backwards of the family
def linear_backward(lin, gy, x, grads, name, params=True):
    """Backward of the dense layer y = x @ W^T + b: returns g_x [B, I] (ops.linear_t); with `params`, the weight / bias gradients
    (ops.dense_wgrad) go into grads[name + ".weight" / ".bias"].  params=False: the data gradient alone (frozen encoder)."""
    W = lin.weight.detach()
    gx = torch.empty((gy.shape[0], W.shape[1]), dtype=torch.float32, device=gy.device)
    ops.linear_t(gy, W, gx)
    if params:
        gw, gb = torch.empty_like(W), torch.empty_like(lin.bias)
        ops.dense_wgrad(gy, x, gw, gb)
        grads[name + ".weight"], grads[name + ".bias"] = gw, gb
    return gx


def fromrgb_param_grads(E, saved, g_out, grads):
    """FromRGB parameter gradients from the gradient of its output (ops.fromrgb_bwd, [C, 4] form)."""
    fr = ops.fromrgb_bwd(g_out, saved["x0"], saved["img"].float())
    grads["FromRGB.from_rgb.weight"] = fr[:, :3].reshape(E.startf, 3, 1, 1)
    grads["FromRGB.from_rgb.bias"] = fr[:, 3]


def grads_in_order(E, grads):
    """`grads` (by parameter name) in E.named_parameters() order: contiguous, or None where there is no gradient."""
    return [g.contiguous() if g is not None else None for g in (grads.get(name) for name, _ in E.named_parameters())]


# ------------------------------------------------------------------ the grouped inver_mod heads
BE_W_ROWS = {"inver_mod1": (1,), "inver_mod2": (0,)}      # E.py:130-134: w[:, 2(L-1-j)] = w2_j, w[:, 2(L-1-j)+1] = w1_j

# one table record per head: the one-column form (dge_heads_fwd / dge_heads_bwd, gcol = row * O) and the row-list form
# (dge_heads_rows_fwd / dge_heads_rows_bwd, one or two rows of w)
_REC_COLUMN = [("W", "u8"), ("moff", "i8"), ("woff", "i8"), ("I", "i4"), ("gcol", "i4"), ("boff", "i4"), ("pad", "i4"), ("bias", "u8")]
_REC_ROWS = [("W", "u8"), ("bias", "u8"), ("moff", "i8"), ("woff", "i8"), ("I", "i4"), ("row_a", "i4"), ("row_b", "i4"), ("boff", "i4")]


def head_list(E, w_rows):
    """The heads that feed W+ as (state_dict name, module, slot, rows): block j owns rows 2(L-1-j) and 2(L-1-j)+1 of w [B, 2L, O]
    (later blocks first), `w_rows` gives each head's row(s) inside that pair; slot 2j = block j's musig1, slot 2j + 1 = musig2."""
    L = E.layer_count
    heads = []
    for j, blk in enumerate(E.decode_block):
        for name, slot in (("inver_mod1", 2 * j), ("inver_mod2", 2 * j + 1)):
            rows = w_rows.get(name)
            if rows:
                heads.append((f"decode_block.{j}.{name}", getattr(blk, name), slot, [2 * (L - 1 - j) + r for r in rows]))
    return heads


def heads_table(E, heads, B, dev, rows):
    """Static layout of the encoder's `inver_mod` heads for the grouped launches, `heads` as head_list gives them.  The (mean, std)
    vectors of all blocks live in one flat buffer, two slots per block of B * I floats; the statistics gradients use the same
    offsets, the parameter gradients another two flat buffers.  The device-side table holds, per head, the weight / bias pointers
    (parameter storage does not move), I, its slot offset, the offsets of its weight / bias gradient and where it sits in w: its
    column (`rows` false: the one-column record) or its one or two rows (`rows` true: the row-list record).
    One layout per (record form, batch size, device), kept while the parameters stay where they are: a captured graph holds the
    address of its table, and a call at another batch size on the same encoder must not free it under that graph."""
    key = (rows, B, str(dev), tuple((h[1].weight.data_ptr(), h[1].bias.data_ptr()) for h in heads))
    cache = E.__dict__.setdefault("_heads_layout", {})
    lay = cache.get(key[:3])
    if lay is not None and lay["key"] == key:
        return lay
    slots, moff = [], 0
    for blk in E.decode_block:
        for _ in range(2):
            slots.append((moff, 2 * blk.inputs)); moff += B * 2 * blk.inputs
    L, O = E.layer_count, heads[0][1].weight.shape[0]
    rec = np.dtype(_REC_ROWS if rows else _REC_COLUMN)
    assert rec.itemsize == (ops.lib().dge_head_rows_entry_size() if rows else ops.lib().dge_head_entry_size())
    tab = np.zeros(len(heads), dtype=rec)
    woff, items = 0, []
    for i, (name, lin, slot, r) in enumerate(heads):
        so, I = slots[slot]
        if tuple(lin.weight.shape) != (O, I) or not lin.weight.is_contiguous() or not 1 <= len(r) <= (2 if rows else 1) or max(r) >= 2 * L:
            raise ops.DgeError(f"heads_table: head {name} does not fit the table (weight {tuple(lin.weight.shape)}, rows {r})")
        if rows:
            tab[i] = (lin.weight.data_ptr(), lin.bias.data_ptr(), so, woff, I, r[0], r[1] if len(r) == 2 else -1, i * O)
        else:
            tab[i] = (lin.weight.data_ptr(), so, woff, I, r[0] * O, i * O, 0, lin.bias.data_ptr())
        items.append((name, slot, woff, i * O, I))
        woff += O * I
    lay = dict(key=key, rows=rows, tab=torch.from_numpy(tab.view(np.uint8).copy()).to(dev), items=items, slots=slots, n=len(heads), O=O,
               total_m=moff, total_w=woff, max_I=max(it[4] for it in items), by_slot={it[1] for it in items})
    cache[key[:3]] = lay
    return lay


def slot_view(lay, flat, i, B):
    """Slot i of a flat statistics buffer (the (mean, std) vectors or their gradients) as [B, I]."""
    so, I = lay["slots"][i]
    return flat[so:so + B * I].view(B, I)


def heads_forward(lay, musig_all, w):
    """Every head of the table in one launch, from the flat (mean, std) buffer into its column / rows of w [B, 2L, O]: none of them
    feeds the trunk, so they run after the last block."""
    (ops.heads_rows_fwd if lay["rows"] else ops.heads_fwd)(lay["tab"], lay["n"], musig_all, w)
    return w


def heads_backward(lay, g_w, musig_all, grads, params=True):
    """Backward of every head at once (their gradient g_w [B, 2L, O] is complete before the backward starts) -> gms_slot(i): the
    gradient of slot i's (mean, std) vector [B, I], None for a slot that feeds no head.  With `params` the weight / bias gradients
    go into `grads` as views of two flat buffers; the one-column kernels always form them."""
    B, O = g_w.shape[0], lay["O"]
    f32 = dict(dtype=torch.float32, device=musig_all.device)
    gms_all = torch.empty(lay["total_m"], **f32)
    gw_all = torch.empty(lay["total_w"], **f32) if params else None
    gb_all = torch.empty(lay["n"] * O, **f32) if params else None
    if lay["rows"]:
        ops.heads_rows_bwd(lay["tab"], lay["n"], lay["max_I"], g_w, musig_all, gms_all, gw_all, gb_all)
    else:
        if not params:
            raise ops.DgeError("heads_backward: the one-column head kernels have no data-gradient-only form")
        if g_w.stride(2) != 1 or g_w.stride(1) != O:
            g_w = g_w.contiguous()
        ops.heads_bwd(lay["tab"], lay["n"], lay["max_I"], g_w, musig_all, gms_all, gw_all, gb_all)
    if params:
        for name, _, woff, boff, I in lay["items"]:
            grads[name + ".weight"] = gw_all[woff:woff + O * I].view(O, I)
            grads[name + ".bias"] = gb_all[boff:boff + O]

    return lambda i: slot_view(lay, gms_all, i, B) if i in lay["by_slot"] else None


# ------------------------------------------------------------------ the block loop and its layer steps
def blocks(E, R, saved=None):
    """j, blk, rec, pre, Cc, C2, H, N per block of a walk at input resolution R.  Forward (no `saved`): every block, rec None.
    With `saved` (a backward): the blocks the forward recorded, last first, rec = that block's saved activations."""
    order = range(len(E.decode_block)) if saved is None else range(len(saved["blocks"]) - 1, -1, -1)
    for j in order:
        blk, H = E.decode_block[j], R >> j
        yield j, blk, (saved["blocks"][j] if saved else None), f"decode_block.{j}.", blk.inputs, blk.outputs, H, H * H


def conv_fwd(cache, blk, k, x, cout, dt, H, sc=None, sh=None, noise=None, act=ops.ACT_LRELU, stats=None):
    """3x3 conv_k of a block on (x * sc + sh), + noise * noise_weight_k (no `noise`: none, E.noise False) + bias_k -> act;
    `stats` receives the result's per-(b,c) sums."""
    return ops.conv2d(x, packed(cache, getattr(blk, f"conv_{k}"), dt, ops.PACK_FWD, H), cout, 3, in_scale=sc, in_shift=sh, noise=noise,
                      noise_w=getattr(blk, f"noise_weight_{k}").detach().reshape(-1) if noise is not None else None,
                      bias=getattr(blk, f"bias_{k}").detach().reshape(-1), act=act, stats=stats)


def red_param_grads(grads, pre, k, red, planar=False, noise=True):
    """bias_k / noise_weight_k gradients from the batch-summed reductions of the activation backward, `red` [C, 2|3] or planar
    [2|3, C] (every row a contiguous view); without `noise` no noise-weight gradient.  -> the third reduction (a caller's sum of
    the incoming gradient), None where red has two."""
    rows = red if planar else red.t()
    Cc = rows.shape[1]
    grads[f"{pre}bias_{k}"] = rows[0].reshape(1, Cc, 1, 1)
    if noise:
        grads[f"{pre}noise_weight_{k}"] = rows[1].reshape(1, Cc, 1, 1)
    return rows[2] if rows.shape[0] == 3 else None


def conv_bwd(cache, grads, name, conv, g, x, dt, H, sc=None, sh=None, params=True, dots=None, dw=None, gain=1.0):
    """Backward of conv `name` (3x3 at resolution H; 1x1 with H None; `gain`: the factor on its output) on (x * sc + sh): the weight
    gradient into grads[name + ".weight"] (`dw`: the caller's zeroed buffer; skipped with params=False), then the data gradient g_x,
    whose epilogue leaves (sum g_x * x, sum g_x) per (b, c) in `dots` (E.BE's ops.SlotStats; None: zeros [B, C, 2] made here; False:
    no sums).  -> (g_x, dots)"""
    if params:
        if dw is None:
            dw = ops.zeros(tuple(conv.weight.shape), g.device)
        ops.conv_wgrad(g, x, dw, sc, sh)
        grads[name + ".weight"] = dw if gain == 1.0 else ops.scale_(dw, gain)
    if dots is None:
        dots = ops.zeros((x.shape[0], x.shape[-1], 2), g.device)
    sums = {} if dots is False else dict(stats=dots, dot_src=x)
    return ops.conv2d(g, packed(cache, conv, dt, ops.PACK_DGRAD, H), x.shape[-1], conv.weight.shape[-1], gain=gain, **sums), dots


def skip_bwd(cache, grads, pre, blk, g_out, xp, dt, bias_sum, params=True, post=None):
    """Backward of the skip branch 0.889 * conv_3(avg_pool(x)) of E.BE / E_Blur from the block's output gradient: conv_3.bias from
    `bias_sum` (the channel sums of g_out; `post`: formed after the caller's deferred sums are flushed), conv_3.weight, then the
    gradient w.r.t. the pooled block input (the caller's `extra`, added with extra_pool and scale 0.25)."""
    if params:
        bias = lambda: grads.__setitem__(pre + "conv_3.bias", bias_sum * 0.889)
        bias() if post is None else post.append(bias)
    return conv_bwd(cache, grads, pre + "conv_3", blk.conv_3, g_out, xp, dt, None, params=params, dots=False, gain=0.889)[0]
