"""StyleGAN2 synthesis pipeline over the HIP ops: forward (reference
model/stylegan2_generator.py:492-539) and the hand-written data-gradient w.r.t. wp that the
encoder training needs (E_align_s2.py:160,204).  G's own parameters never receive gradients
here: the reference computes and discards them, results for E are identical."""
import torch

from . import ops, s2_conv
from .stylegan2_generator import _dt
from .weight_cache import version


def style_groups(mod):
    """[(modulated block, its row of wp)] in the order of the flat style buffer: the conv layers, then the toRGB blocks."""
    nl = mod.num_layers
    return [(getattr(mod, f"layer{i}"), i) for i in range(nl - 1)] + [(getattr(mod, f"output{k}"), 2 * k + 1) for k in range(nl // 2)]


def _style_tables(mod, B, dt):
    """Row-concatenated style weights / demodulation tables of all 17 + 9 modulated blocks (cached; G is frozen in E_align)
    so that every style vector and demodulation factor of a pass comes from two launches (dge_linear_rows, dge_demod_rows).
    One entry per (batch size, dtype), kept while the weights stay as they are: a captured graph holds the addresses of the index
    tables of its batch size, and a step at another batch size on the same generator must not free them under it (the next
    replay of the first graph would index through freed memory)."""
    nl = mod.num_layers
    groups = style_groups(mod)
    key = (B, str(dt)) + tuple(version(p) for L, _ in groups for p in (L.style.weight, L.style.bias, L.weight))
    cache = mod.__dict__.setdefault("_style_tab", {})
    hit = cache.get(key[:2])
    if hit is not None and hit[0] == key:
        return hit[1]
    dev = groups[0][0].weight.device
    K = mod.w_space_dim
    Wc = torch.cat([L.style.weight.detach() for L, _ in groups]).contiguous()
    bc = torch.cat([L.style.bias.detach() for L, _ in groups]).contiguous()
    xoff, ybase, ybs, s_off = [], [], [], []
    off = 0
    for L, row in groups:
        C = L.in_c
        s_off.append(B * off)
        xoff += [row * K] * C
        ybase += [B * off + c for c in range(C)]
        ybs += [C] * C
        off += C
    woff, sbase, cin, dbase, dbs, d_off, wsq = [], [], [], [], [], [], []
    doff, wpos = 0, 0
    for gi, (L, _) in enumerate(groups[:nl - 1]):
        _, wq = L._prepared(dt)
        wsq.append(wq.reshape(-1))
        d_off.append(B * doff)
        for o in range(L.out_c):
            woff.append(wpos + o * L.in_c); sbase.append(s_off[gi]); cin.append(L.in_c)
            dbase.append(B * doff + o); dbs.append(L.out_c)
        doff += L.out_c
        wpos += L.out_c * L.in_c
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    st0 = groups[0][0].style
    for L, _ in groups:
        assert L.style.wscale == st0.wscale and L.style.bscale == st0.bscale and L.style.additional_bias == st0.additional_bias
    tab = dict(groups=groups, Wc=Wc, bc=bc, xoff=i32(xoff), ybase=i32(ybase), ybs=i32(ybs), s_off=s_off, s_total=B * off,
               wsq=torch.cat(wsq).contiguous(), woff=i32(woff), sbase=i32(sbase), cin=i32(cin), dbase=i32(dbase), dbs=i32(dbs),
               d_off=d_off, d_total=B * doff, wscale=st0.wscale, bscale=st0.bscale, add=st0.additional_bias, eps=groups[0][0].eps)
    cache[key[:2]] = (key, tab)
    return tab


def check_noises(mod, noises, B, device):
    """`noises` of synthesis(): one f32 map [1,res,res] (shared by the batch) or [B,res,res] (a map per row) per conv layer, in layer
    order, contiguous, on the device - what the kernels' noise operand (batch stride 0 or res^2) takes as it is."""
    noises = list(noises)
    if len(noises) != mod.num_layers - 1:
        raise ValueError(f"synthesis: `noises` takes one map per conv layer ({mod.num_layers - 1}), got {len(noises)}")
    for i, n in enumerate(noises):
        res = getattr(mod, f"layer{i}").res
        if not torch.is_tensor(n) or n.dtype != torch.float32 or n.dim() != 3 or tuple(n.shape[1:]) != (res, res) or n.shape[0] not in (1, B):
            raise ValueError(f"synthesis: noises[{i}] must be a float32 tensor [1,{res},{res}] or [{B},{res},{res}]")
        if not n.is_contiguous() or n.device != device:
            raise ValueError(f"synthesis: noises[{i}] must be contiguous and on {device}")
    return noises


def styles_from_wp(mod, wp, out=None, tab=None):
    """Every style vector of the pass from wp [B,L,512] in one launch (dge_linear_rows) -> the flat f32 buffer of _style_tables'
    layout for batch B (block g at B * off_g, viewed [B,C_g]); `out`: written in place."""
    B = wp.shape[0]
    tab = _style_tables(mod, B, _dt(mod.compute_dtype)) if tab is None else tab
    wpc = wp if (wp.dtype == torch.float32 and wp.is_contiguous()) else wp.float().contiguous()
    s_all = torch.empty(tab["s_total"], dtype=torch.float32, device=wp.device) if out is None else out
    ops.linear_rows(wpc, mod.num_layers * mod.w_space_dim, tab["xoff"], tab["Wc"], tab["bc"], s_all, tab["ybase"], tab["ybs"], B,
                    tab["wscale"], tab["bscale"], tab["add"])
    return s_all


def styles_batch(mod, styles):
    """The batch size a flat style buffer `styles` holds (ValueError where it is no such buffer)."""
    per_row = sum(L.in_c for L, _ in style_groups(mod))
    if (not torch.is_tensor(styles) or styles.dtype != torch.float32 or styles.dim() != 1 or styles.numel() == 0 or styles.numel() % per_row
            or not styles.is_contiguous()):
        raise ValueError(f"synthesis: `styles` is a StyleCodes or its flat tensor: contiguous float32 [B * {per_row}]")
    return styles.numel() // per_row


def synthesis_run(mod, wp, randomize_noise=False, save=False, noises=None, styles=None):
    """`styles` (with wp None): the flat style buffer in place of the one dge_linear_rows fills from wp."""
    dt = _dt(mod.compute_dtype)
    nl = mod.num_layers
    # ---- all styles and demodulation factors of the pass: two launches instead of 2*17 + 9
    if styles is None:
        B = wp.shape[0]
        results = {"wp": wp}
        tab = _style_tables(mod, B, dt)
        s_all = styles_from_wp(mod, wp, tab=tab)
    else:
        B = styles_batch(mod, styles)
        results = {}
        tab = _style_tables(mod, B, dt)
        wp = s_all = styles
    d_all = torch.empty(tab["d_total"], dtype=torch.float32, device=wp.device)
    ops.demod_rows(s_all, tab["wsq"], tab["woff"], tab["sbase"], tab["cin"], d_all, tab["dbase"], tab["dbs"], B, tab["eps"])
    s_of = lambda g, C: s_all[tab["s_off"][g]:tab["s_off"][g] + B * C].view(B, C)
    x = ops.nchw_to_nhwc(mod.early_layer.const.detach(), B, dt)
    saved = {"const": x, "layers": [], "rgb": []} if save else None
    image = None
    for i in range(nl - 1):
        L = getattr(mod, f"layer{i}")
        s = s_of(i, L.in_c)
        d = d_all[tab["d_off"][i]:tab["d_off"][i] + B * L.out_c].view(B, L.out_c)
        if noises is not None:
            noise = noises[i].detach()
        elif randomize_noise:
            noise = ops.randn((x.shape[0], L.res, L.res), x.device)
        else:
            noise = L.noise.reshape(1, L.res, L.res)
        # the toRGB of the top layers rides in their conv epilogue where the streaming kernel offers it (512^2 / 1024^2: the activation
        # is not read back by a toRGB pass, and the last one is not even written when nothing else reads it); the skip image is
        # added afterwards
        fuse_rgb = (i % 2 == 0 and image is not None and not L.up and L.bias is not None and
                    ops.conv_rgb_supported(B, L.res, L.res, L.in_c, L.out_c, 3, dt))
        rgb = None
        if fuse_rgb:
            O_ = getattr(mod, f"output{i // 2}")
            srgb = s_of(nl - 1 + i // 2, O_.in_c)
            rgb = dict(w=O_.weight.detach().reshape(3, -1), style=srgb, bias=O_.bias.detach(), wscale=O_.wscale,
                       out=torch.empty((B, 3, L.res, L.res), dtype=torch.float32, device=x.device), skip_y=(not save) and i == nl - 2)
        y = L.conv(x, s, d, noise, dt, rgb=rgb)
        results[f"style{i:02d}"] = s
        if save:
            saved["layers"].append(dict(y=y, s=s, d=d, noise=noise))
        x = y
        if fuse_rgb:
            image = ops.rgb_upsample_add(rgb["out"], image)
            results[f"output_style{i // 2}"] = srgb
            if save:
                saved["rgb"].append(dict(s=srgb))
        elif i % 2 == 0:
            O_ = getattr(mod, f"output{i // 2}")
            srgb = s_of(nl - 1 + i // 2, O_.in_c)
            image = ops.torgb(x, O_.weight, srgb, O_.bias, image, O_.wscale)
            results[f"output_style{i // 2}"] = srgb
            if save:
                saved["rgb"].append(dict(s=srgb))
    results["image"] = image
    return results, saved


def _torgb_adjoint(mod, saved, i, g_img, x_in, emit):
    """The toRGB block that reads x_in, the output of layer i - 1 (even layers carry one): (its gradient w.r.t. x_in - the addend
    of layer i's data gradient - or None, g_img brought down to the resolution of the block below).  The block's style gradient goes
    to emit(g_srgb, block, row of g_wp)."""
    if i < 1 or (i - 1) % 2:
        return None, g_img
    k = (i - 1) // 2
    O = getattr(mod, f"output{k}")
    addend, g_srgb = ops.torgb_bwd(g_img, x_in, O.weight.detach().reshape(3, -1), saved["rgb"][k]["s"], O.wscale)
    emit(g_srgb, O, i)
    return addend, (ops.up2_bwd(g_img) if k > 0 else g_img)


def _style_grads(L, rec, dt, R, st, g_wp_row):
    """style / demodulation gradients of a layer whose tail backward ran as a pass of its own (sums in R), st [B,in_c,2] -> g_wp[:, i]
    (g_wp_row None, the S form: the layer stops at g_s = st[..., 0], which dge_s2_style_grads_s brings to the block's slice)"""
    B = st.shape[0]
    t = ops.demod_bwd(R, rec["d"], L.bias.detach(), L.noise_strength.detach().reshape(1), L.bscale)
    gs_view = st.view(B, -1)      # [B, 2*Cin]: element (b, 2*i) = g_s[b,i]
    ops.linear_t(t, L._prepared(dt)[1], gs_view, mul=rec["s"], accumulate=True, incy=2, ldy=2 * L.in_c)
    if g_wp_row is not None:
        ops.linear_t(gs_view, L.style.weight.detach(), g_wp_row, scale=L.style.wscale, accumulate=True, incx=2, ldx=2 * L.in_c, O=L.in_c)


def _noise_grad(ng, i, L, rec, g, z_form):
    """g_noise of layer i where asked for (ng: {layer: out [Bn, res^2] f32}, None: nowhere): from g_z as it is (`z_form`, form A),
    else from the gradient w.r.t. the layer output, the kernel applying gain * lrelu'(x) (form B)."""
    if ng and i in ng:
        ops.s2_noise_grad(g, None if z_form else rec["y"], L.gain, L.noise_strength.detach().reshape(1), ng[i])


def _backward_fused(mod, saved, g_img, g_wp, dt, ng=None, gs=None):
    """Atomics mode.  The gradient travels down the chain as g_z, w.r.t. the pre-activation of each layer: the data-gradient launch
    of layer i + 1 differentiates layer i's noise / bias / lrelu tail in its own epilogue (`prep`: it streams layer i's stored
    output as dot_src anyway) and leaves the two per-(b,c) sums of the demodulation gradient in P; the demodulation factor d
    multiplies g_z in the NEXT launch.  Every style gradient leaves in ONE launch at the end (dge_s2_style_grads): none feeds the
    chain.  Where the route of layer i + 1 does not take prep (s2_conv.dgrad_route), layer i runs its tail as a pass of its own and
    finishes its style gradient as the deterministic chain does.
    S form (`gs`: every block's [B,in_c] slice of the style-gradient buffer in the order of style_groups, g_wp None): the same
    chain and the same `blocks`, each with its slice in place of (wstyle, row), end in dge_s2_style_grads_s."""
    B, dev, layers, top = g_img.shape[0], g_img.device, saved["layers"], mod.num_layers - 2
    blocks = []
    if gs is None:
        emit = lambda g_srgb, O, row: blocks.append(dict(gs=g_srgb, wstyle=O.style.weight.detach(), row=row))
        dest = lambda L, i: dict(wstyle=L.style.weight.detach(), row=i)
    else:
        emit = lambda g_srgb, O, row: blocks.append(dict(gs=g_srgb, out=gs[top + 1 + (row - 1) // 2]))          # (toRGB k: row 2k + 1)
        dest = lambda L, i: dict(out=gs[i])
    # top layer: its output only feeds the last toRGB (image_k = rgb_k + up(image_{k-1}), :515-522)
    Lt, Ot = getattr(mod, f"layer{top}"), getattr(mod, f"output{top // 2}")
    g_x, g_srgb, P = ops.torgb_bwd_prep(g_img, layers[top]["y"], Ot.weight.detach().reshape(3, -1), saved["rgb"][top // 2]["s"], Ot.wscale,
                                        layers[top]["noise"], Lt.noise_strength.detach().reshape(1), Lt.gain)
    emit(g_srgb, Ot, top + 1)
    if top // 2 > 0:
        g_img = ops.up2_bwd(g_img)
    for i in range(top, -1, -1):
        L, rec = getattr(mod, f"layer{i}"), layers[i]
        _noise_grad(ng, i, L, rec, g_x, P is not None)
        if P is not None:
            g_y, d_in = g_x, rec["d"]                  # g_x is g_z already (with its sums in P); d joins in the launch
        else:
            R = ops.zeros((B, L.out_c, 3), dev)
            g_y, d_in = ops.modconv_bwd_prep(g_x, rec["y"], rec["d"], rec["noise"], L.gain, R), None
        x_in = saved["const"] if i == 0 else layers[i - 1]["y"]
        addend, g_img = _torgb_adjoint(mod, saved, i, g_img, x_in, emit)
        st = ops.SlotStats(B, L.in_c, dev)
        route = s2_conv.dgrad_route(L, B, dt, True, d_in is not None)
        prep, P_next = None, None
        if route.takes_prep and i >= 1:
            Lp = getattr(mod, f"layer{i - 1}")
            P_next = ops.SlotStats(B, L.in_c, dev)
            prep = dict(gain=Lp.gain, noise=layers[i - 1]["noise"], ns=Lp.noise_strength.detach().reshape(1), stats=P_next)
        g_x = s2_conv.dgrad(L, route, g_y, d_in, dt, prep, rec["s"], addend, st, x_in)
        if P is not None:
            blocks.append(dict(P=P, st=st, d=rec["d"], s=rec["s"], bias=L.bias.detach(), wsq=L._prepared(dt)[1], bscale=L.bscale,
                               **dest(L, i)))
        else:
            st1 = ops.sum_slots(st.buf, ops.zeros((B, L.in_c, 2), dev), accumulate=False)
            _style_grads(L, rec, dt, R, st1, None if gs is not None else g_wp[:, i])
            if gs is not None:
                blocks.append(dict(st=st1, out=gs[i]))
        P = P_next
    if gs is not None:
        ops.s2_style_grads_s(blocks, B)
    else:
        ops.s2_style_grads(blocks, g_wp, getattr(mod, "layer0").style.wscale)


def _backward_det(mod, saved, g_img, g_wp, dt, ng=None, gs=None):
    """Deterministic mode: the same math with no atomics.  The gradient travels as g_x, w.r.t. each layer's output; the tail backward
    is a pass of its own per layer (dge_modconv_bwd_prep, which applies d), and each layer's style gradient is finished on the spot.
    S form (`gs` as in _backward_fused): every layer stops at g_s, and one dge_s2_style_grads_s launch at the end brings the g_s of
    all blocks to their slices (plain stores, one writer per element)."""
    B, dev, layers, top = g_img.shape[0], g_img.device, saved["layers"], mod.num_layers - 2
    blocks = []
    if gs is None:
        emit = lambda g_srgb, O, row: ops.linear_t(g_srgb, O.style.weight.detach(), g_wp[:, row], scale=O.style.wscale, accumulate=True)
    else:
        emit = lambda g_srgb, O, row: blocks.append(dict(gs=g_srgb, out=gs[top + 1 + (row - 1) // 2]))
    # top layer: its output only feeds the last toRGB (image_k = rgb_k + up(image_{k-1}), :515-522)
    Ot = getattr(mod, f"output{top // 2}")
    g_x, g_srgb = ops.torgb_bwd(g_img, layers[top]["y"], Ot.weight.detach().reshape(3, -1), saved["rgb"][top // 2]["s"], Ot.wscale)
    emit(g_srgb, Ot, top + 1)
    if top // 2 > 0:
        g_img = ops.up2_bwd(g_img)
    for i in range(top, -1, -1):
        L, rec = getattr(mod, f"layer{i}"), layers[i]
        _noise_grad(ng, i, L, rec, g_x, False)
        R = ops.zeros((B, L.out_c, 3), dev)
        g_y = ops.modconv_bwd_prep(g_x, rec["y"], rec["d"], rec["noise"], L.gain, R)
        x_in = saved["const"] if i == 0 else layers[i - 1]["y"]
        addend, g_img = _torgb_adjoint(mod, saved, i, g_img, x_in, emit)
        st = ops.zeros((B, L.in_c, 2), dev)
        g_x = s2_conv.dgrad(L, s2_conv.dgrad_route(L, B, dt, False, False), g_y, None, dt, None, rec["s"], addend, st, x_in)
        _style_grads(L, rec, dt, R, st, None if gs is not None else g_wp[:, i])
        if gs is not None:
            blocks.append(dict(st=st, out=gs[i]))
    if gs is not None:
        ops.s2_style_grads_s(blocks, B)


def synthesis_backward(mod, wp, saved, g_image, noise_grads=None, style_grads=None):
    """d(image)/d(wp) contracted with g_image [B,3,R,R] -> g_wp [B,num_layers,512], layer by layer from the top (the pre-activation
    of a layer is z = yraw*d + noise*ns + bias, stylegan2_generator.py:908-921), in the form of the library's mode.
    `noise_grads`: {conv layer: f32 [Bn, res^2]} to receive the gradient w.r.t. that layer's noise map (Bn 1: the map is shared by
    the batch) - a pass of its own per entry beside the chain (dge_s2_noise_grad), which runs exactly as it does without.
    `style_grads` (the S form, for a pass that ran on `styles`; wp is ignored): the flat f32 buffer of the styles' layout that
    receives d(image)/d(styles) contracted with g_image, every element written once; no g_wp is allocated, and it is what returns."""
    chain = _backward_det if ops.is_deterministic() else _backward_fused
    if style_grads is not None:
        B, off, gs = g_image.shape[0], 0, []
        for L, _ in style_groups(mod):
            gs.append(style_grads[B * off:B * (off + L.in_c)].view(B, L.in_c))
            off += L.in_c
        if style_grads.numel() != B * off or style_grads.dtype != torch.float32 or not style_grads.is_contiguous():
            raise ValueError(f"synthesis: the style-gradient buffer must be contiguous float32 [{B * off}]")
        chain(mod, saved, g_image.float().contiguous(), None, ops.dtype_of(saved["const"]), noise_grads, gs)
        return style_grads
    g_wp = ops.zeros((wp.shape[0], mod.num_layers, mod.w_space_dim), wp.device)
    chain(mod, saved, g_image.float().contiguous(), g_wp, ops.dtype_of(saved["const"]), noise_grads)
    return g_wp


class StyleGradOut:
    """grad_out of SynthesisFunction in S form: `noises` = noise_grad_out, `styles` = style_grad_out (either may be None)."""
    __slots__ = ("noises", "styles")

    def __init__(self, noises, styles):
        self.noises, self.styles = noises, styles


class SynthesisFunction(torch.autograd.Function):
    """Inputs behind `keys`: `grad_out` (None, or per conv layer None or an f32 buffer of the map's shape: the backward writes that
    layer's noise gradient THERE instead of returning it to autograd - static storage for a captured iteration, no accumulation
    pass) and the noise maps, if any.  S form: `wp` is the flat style buffer and `grad_out` a StyleGradOut around the two
    destinations, the noise maps' list and the flat buffer for the style gradient (None: it returns to autograd)."""

    @staticmethod
    def forward(ctx, mod, wp, randomize_noise, keys, grad_out, *noises):
        need = any(ctx.needs_input_grad)
        ctx.s_form = isinstance(grad_out, StyleGradOut)
        ctx.style_out = grad_out.styles if ctx.s_form else None
        if ctx.s_form:
            grad_out = grad_out.noises
            results, saved = synthesis_run(mod, None, randomize_noise, save=need, noises=noises or None, styles=wp.detach())
        else:
            results, saved = synthesis_run(mod, wp.detach(), randomize_noise, save=need, noises=noises or None)
        ctx.mod, ctx.saved_acts, ctx.wp = mod, saved, wp.detach()
        ctx.grad_out, ctx.noise_shapes = grad_out, [tuple(n.shape) for n in noises]
        keys += [k for k in results if k not in ("wp", "image")]          # (the caller's list: the order synthesis_run produced)
        outs = [results[k] for k in keys]
        ctx.mark_non_differentiable(*outs)
        return (results["image"], *outs)

    @staticmethod
    def backward(ctx, g_image, *unused):
        if ctx.saved_acts is None:
            raise RuntimeError("synthesis was run without saved activations")
        ng, ret = {}, [None] * len(ctx.noise_shapes)
        if ctx.mod.noise_grad_enabled:          # (read here: a second backward through the same graph may switch the passes off)
            for i, shape in enumerate(ctx.noise_shapes):
                if ctx.needs_input_grad[5 + i]:
                    out = ctx.grad_out[i] if ctx.grad_out is not None else None
                    if out is None:
                        ng[i] = ret[i] = torch.empty(shape, dtype=torch.float32, device=g_image.device)
                    elif tuple(out.shape) != shape or out.dtype != torch.float32:
                        raise ValueError(f"synthesis: noise_grad_out[{i}] must be float32 {shape}")
                    else:
                        ng[i] = out
        if ctx.s_form:
            out = ctx.style_out if ctx.style_out is not None else torch.empty_like(ctx.wp)
            synthesis_backward(ctx.mod, None, ctx.saved_acts, g_image, ng, style_grads=out)
            return (None, None if ctx.style_out is not None else out, None, None, None, *ret)
        g_wp = synthesis_backward(ctx.mod, ctx.wp, ctx.saved_acts, g_image, ng)
        return (None, g_wp, None, None, None, *ret)


def synthesis_forward(mod, wp, randomize_noise=False, noises=None, noise_grad_out=None, styles=None, style_grad_out=None):
    """SynthesisModule.forward: conv layer i is driven by wp[:, i]; the toRGB of block k by
    wp[:, 2k+1] (reference :511-517).  Returns the reference's result dict.  `noises`: the conv layers' noise maps in place of the
    `layer{i}.noise` buffers (check_noises); the image is differentiable w.r.t. every map that requires grad.
    `styles` (a StyleCodes or its flat tensor, with wp None): the pass starts from the style vectors themselves (_synthesis_styles)."""
    if styles is not None or style_grad_out is not None:
        return _synthesis_styles(mod, wp, randomize_noise, noises, noise_grad_out, styles, style_grad_out)
    wp = wp if (wp.dtype == torch.float32 and wp.is_contiguous()) else wp.float().contiguous()
    if noises is not None:
        if randomize_noise:
            raise ValueError("synthesis: `noises` fixes every noise map; randomize_noise=True contradicts it")
        noises = check_noises(mod, noises, wp.shape[0], wp.device)
    if noise_grad_out is not None and (noises is None or len(noise_grad_out) != len(noises)):
        raise ValueError("synthesis: noise_grad_out takes one buffer (or None) per map of `noises`")
    if torch.is_grad_enabled() and (wp.requires_grad or any(n.requires_grad for n in noises or ())):
        keys = []
        image, *outs = SynthesisFunction.apply(mod, wp, randomize_noise, keys, noise_grad_out, *(noises or ()))
        return {"wp": wp, **dict(zip(keys, outs)), "image": image}
    results, _ = synthesis_run(mod, wp, randomize_noise, save=False, noises=noises)
    return results


def _synthesis_styles(mod, wp, randomize_noise, noises, noise_grad_out, styles, style_grad_out):
    """synthesis(styles=...): the S code as the input of the pass.  No dge_linear_rows: the flat buffer feeds dge_demod_rows and the
    layers as s_all does.  The result dict holds the image and the style views, and no wp.  Where the flat tensor requires grad the
    backward ends in S form (synthesis_backward(style_grads=...)); `style_grad_out`: a flat f32 buffer of the styles' layout that
    the gradient is written to INSTEAD of reaching .grad (noise_grad_out's convention, for a captured iteration)."""
    if styles is None:
        raise ValueError("synthesis: style_grad_out needs `styles`: it receives the gradient of the style codes")
    if wp is not None:
        raise ValueError("synthesis: `styles` takes the place of wp: pass wp=None with it (the styles are not recomputed from wp)")
    flat = getattr(styles, "flat", styles)
    B = styles_batch(mod, flat)
    if not flat.is_cuda:
        raise ValueError("synthesis: `styles` must be on the GPU")
    if noises is not None:
        if randomize_noise:
            raise ValueError("synthesis: `noises` fixes every noise map; randomize_noise=True contradicts it")
        noises = check_noises(mod, noises, B, flat.device)
    if noise_grad_out is not None and (noises is None or len(noise_grad_out) != len(noises)):
        raise ValueError("synthesis: noise_grad_out takes one buffer (or None) per map of `noises`")
    if style_grad_out is not None and (not torch.is_tensor(style_grad_out) or tuple(style_grad_out.shape) != tuple(flat.shape)
                                       or style_grad_out.dtype != torch.float32 or not style_grad_out.is_contiguous()
                                       or style_grad_out.device != flat.device):
        raise ValueError(f"synthesis: style_grad_out must be a contiguous float32 buffer {tuple(flat.shape)} on {flat.device}")
    if torch.is_grad_enabled() and (flat.requires_grad or any(n.requires_grad for n in noises or ())):
        keys = []
        image, *outs = SynthesisFunction.apply(mod, flat, randomize_noise, keys, StyleGradOut(noise_grad_out, style_grad_out), *(noises or ()))
        return {**dict(zip(keys, outs)), "image": image}
    results, _ = synthesis_run(mod, None, randomize_noise, save=False, noises=noises, styles=flat.detach())
    return results
