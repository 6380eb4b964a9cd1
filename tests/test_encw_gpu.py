"""Ablations 3 and 2 on the GPU (dge_amd.e_align_w): the grouped head kernels with a row list (dge_heads_rows_fwd / _bwd) alone,
the E_Blur_W / E_Blur_W_2 encoders against the reference's gradients (tests/golden/encw_grad.npz) and the two-phase loop against the
reference's own runs of 3.E_align_w.py and 2.E_align_w_2.py at reduced size (step_w.npz, step_w2.npz; tools/gen_golden.py sections
encw_grad, step_w, step_w2)."""
import numpy as np
import pytest
import torch

from tests.conftest import golden, with_fixture_params, meas, MODES
from tests.golden import recipe as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def relerr(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    return ((a - b).abs().max() / b.abs().max()).item()


def _l2rel(a, b):
    a = a.detach().float().cpu().flatten(); b = torch.as_tensor(np.asarray(b)).float().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _cls(variant):
    from dge_amd.encoder_variants import BlurBEW, BlurBEW2
    return {"w": BlurBEW, "w_2": BlurBEW2}[variant]


# ----------------------------------------------------------------------------------------------------------------- kernels
HEAD_I = (32, 64, 192, 1024)                    # 32: below one wave; 192 / 1024: several lane strides, 3 / 16 column blocks
HEAD_ROWS = ((0,), (1, 2), (3,), (4, 5))        # one-row and two-row entries mixed; every row of the 6 owned by exactly one head


def _head_case(B, O):
    """-> (table, weights, biases, musig per head, flat musig, offsets): one launch's worth of heads, bias non-zero"""
    from dge_amd import ops
    rec = np.dtype([("W", "u8"), ("bias", "u8"), ("moff", "i8"), ("woff", "i8"), ("I", "i4"), ("row_a", "i4"), ("row_b", "i4"), ("boff", "i4")])
    assert rec.itemsize == ops.lib().dge_head_rows_entry_size()
    Ws = [R.randn(f"hr.W{i}", (O, I), 3, 1.0 / I ** 0.5).to(DEV) for i, I in enumerate(HEAD_I)]
    bs = [R.randn(f"hr.b{i}", (O,), 3, 0.3).to(DEV) for i in range(len(HEAD_I))]
    ms = [R.randn(f"hr.m{i}", (B, I), 4).to(DEV) for i, I in enumerate(HEAD_I)]
    tab = np.zeros(len(HEAD_I), dtype=rec)
    moff = woff = 0
    offs = []
    for i, I in enumerate(HEAD_I):
        rows = HEAD_ROWS[i]
        tab[i] = (Ws[i].data_ptr(), bs[i].data_ptr(), moff, woff, I, rows[0], rows[1] if len(rows) == 2 else -1, i * O)
        offs.append((moff, woff, i * O))
        moff += B * I
        woff += O * I
    musig_all = torch.cat([m.reshape(-1) for m in ms])
    return torch.from_numpy(tab.view(np.uint8).copy()).to(DEV), Ws, bs, ms, musig_all, offs, woff


def _strided_rows(B, O, fill):
    """a [B, 6, O] view with unit inner stride inside a larger tensor (row stride O + 24, rows 1..6 of 8, columns 8..8+O)"""
    big = torch.full((B, 8, O + 24), fill, dtype=torch.float32, device=DEV)
    return big, big[:, 1:7, 8:8 + O]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("O", [512, 40])
def test_heads_rows_fwd_is_bit_identical_to_linear_and_writes_every_row_once(B, O):
    from dge_amd import ops
    tab, Ws, bs, ms, musig_all, _, _ = _head_case(B, O)
    big, w = _strided_rows(B, O, float("nan"))
    assert not w.is_contiguous() and w.stride(2) == 1
    ops.heads_rows_fwd(tab, len(HEAD_I), musig_all, w)
    assert torch.isfinite(w).all()                               # every row of the view written
    outside = big.clone()
    outside[:, 1:7, 8:8 + O] = float("nan")
    assert torch.isnan(outside).all() and torch.isnan(big[:, 0]).all() and torch.isnan(big[:, 7]).all()      # and nothing else
    seen = []
    for i, rows in enumerate(HEAD_ROWS):
        ref = ops.linear(ms[i], Ws[i], bs[i])
        for r in rows:
            assert torch.equal(w[:, r], ref), (i, r)
            seen.append(r)
    assert sorted(seen) == list(range(6))
    # a contiguous destination gives the same bits
    wc = torch.empty((B, 6, O), device=DEV)
    ops.heads_rows_fwd(tab, len(HEAD_I), musig_all, wc)
    assert torch.equal(wc, w)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("O", [512, 40])
def test_heads_rows_bwd_vs_float64_products_and_is_reproducible(B, O):
    """gms = g @ W, gW = g^T @ musig, gb = sum_b g with g = g_w[:, row_a] (+ g_w[:, row_b]), against the same products in float64
    on the host from the same inputs: 1e-5 of the tensor's max (the bound of test_mapping_dz_* for f32 dense products of this
    length: at most 1024 terms per sum, ~sqrt(1024) * 2^-24 = 2e-6 of the typical magnitude)."""
    from dge_amd import ops
    tab, Ws, bs, ms, musig_all, offs, total_w = _head_case(B, O)
    big, g = _strided_rows(B, O, 7.0)
    g.copy_(R.randn("hr.g", (B, 6, O), 5).to(DEV))
    n = len(HEAD_I)

    def run(params):
        gms = torch.full((musig_all.numel(),), float("nan"), device=DEV)
        gw = torch.full((total_w,), float("nan"), device=DEV) if params else None
        gb = torch.full((n * O,), float("nan"), device=DEV) if params else None
        ops.heads_rows_bwd(tab, n, max(HEAD_I), g, musig_all if params else None, gms, gw, gb)
        return gms, gw, gb
    gms, gw, gb = run(True)
    gms2, gw2, gb2 = run(True)
    assert torch.equal(gms, gms2) and torch.equal(gw, gw2) and torch.equal(gb, gb2)          # no atomics: the same bits
    gms_d, none_w, none_b = run(False)                                                       # the data gradient alone
    assert none_w is None and none_b is None and torch.equal(gms_d, gms)
    assert torch.isfinite(gms).all() and torch.isfinite(gw).all() and torch.isfinite(gb).all()      # every element written
    gh = g.double().cpu()
    worst = dict(gms=0.0, gW=0.0, gb=0.0)
    for i, I in enumerate(HEAD_I):
        rows = HEAD_ROWS[i]
        gl = gh[:, rows[0]] + (gh[:, rows[1]] if len(rows) == 2 else 0.0)
        moff, woff, boff = offs[i]
        for name, mine, ref in (("gms", gms[moff:moff + B * I].view(B, I), gl @ Ws[i].double().cpu()),
                                ("gW", gw[woff:woff + O * I].view(O, I), gl.t() @ ms[i].double().cpu()),
                                ("gb", gb[boff:boff + O], gl.sum(0))):
            e = relerr(mine, ref)
            worst[name] = max(worst[name], e)
            assert e <= 1e-5, (i, name, e)
    meas("heads_rows_bwd", B=B, O=O, **worst)
    # the input view's surroundings were only read
    assert float(big[:, 0].min()) == 7.0 and float(big[:, 7].max()) == 7.0


def test_wrappers_refuse_what_the_kernels_do_not_address():
    from dge_amd import ops
    tab, Ws, bs, ms, musig_all, offs, total_w = _head_case(1, 40)
    with pytest.raises(ops.DgeError, match="unit inner stride"):
        ops.heads_rows_fwd(tab, 4, musig_all, torch.empty((1, 40, 6), device=DEV).transpose(1, 2))
    g = torch.zeros((1, 6, 2048), device=DEV)
    with pytest.raises(ops.DgeError, match="O <= 1024"):
        ops.heads_rows_bwd(tab, 4, 1024, g, None, torch.empty(musig_all.numel(), device=DEV))


# ----------------------------------------------------------------------------------------------------------------- encoders
def _encw(variant, cd):
    g = golden("encw_grad.npz")
    E = _cls(variant)(startf=32, maxf=512, layer_count=5, compute_dtype=cd).cuda()
    sd = R.fill_encoder({k: list(v.shape) for k, v in E.state_dict().items()}, seed=81)
    for k in sd:
        if k.endswith("blur.weight"):
            sd[k] = E.state_dict()[k].clone()
    E.load_state_dict(with_fixture_params(sd, g))
    return E, g


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cd", ["f32", "bf16"])
@pytest.mark.parametrize("variant", ["w", "w_2"])
def test_e_blur_w_gradients_vs_reference_golden(variant, cd, mode):
    """Structure and bounds of test_e_blur_z_gradients_vs_reference_golden (the project's bounds for this trunk)."""
    E, g = _encw(variant, cd)
    img = R.randn("ew.img", (2, 3, 64, 64), 81, 0.5).cuda().requires_grad_(True)
    x, w = E(img)
    assert tuple(x.shape) == (2, 512, 4, 4) and tuple(w.shape) == (2, 10, 512)
    xerr, werr = relerr(x, g["x"]), relerr(w, g[f"{variant}:w"])
    loss = (x * R.randn("ew.gx", tuple(x.shape), 83).cuda()).sum() + (w * R.randn("ew.gw", tuple(w.shape), 84).cuda()).sum()
    loss.backward()
    f32 = cd == "f32"
    tol, tol_img = (1e-3, 1e-3) if f32 else (0.48, 0.43)
    worst, checked = (0.0, None), 0
    for k, p in E.named_parameters():
        if f"{variant}:grad:{k}" not in g.files:
            assert p.grad is None, k                         # no gradient in the reference: none here (not zeros)
            continue
        nrm = float(g[f"{variant}:norm:{k}"])
        mine = p.grad.detach().float().cpu()
        assert abs(float(mine.norm()) - nrm) < tol * nrm + 1e-6, (k, float(mine.norm()), nrm)
        ref = g[f"{variant}:grad:{k}"]
        mine = mine if mine.numel() == ref.size else mine.flatten()[:ref.size]
        e = _l2rel(mine, ref)
        worst = max(worst, (e, k))
        assert e < tol, (k, e)
        checked += 1
    img_e = _l2rel(img.grad, g[f"{variant}:g_img"])
    meas("encw_grads", variant=variant, cd=cd, mode=mode, x=xerr, w=werr, worst_l2=worst[0], key=worst[1], img_l2=img_e, checked=checked)
    assert xerr < (2e-4 if f32 else 3e-2) and werr < (2e-4 if f32 else 3e-2), (xerr, werr)
    assert checked >= 30 and img_e < tol_img, (checked, img_e)
    if variant == "w_2":
        for k, p in E.named_parameters():
            if "inver_mod1" in k:
                assert p.grad is None, k
        # (inver_mod2.weight's gradient above matches the reference's only as the sum of the two row gradients)
        assert f"{variant}:grad:decode_block.4.inver_mod2.weight" in g.files
        for k in range(5):
            assert torch.equal(w[:, 2 * k], w[:, 2 * k + 1]), k
    else:
        assert E.decode_block[0].inver_mod1.weight.grad is not None
        assert not torch.equal(w[:, 0], w[:, 1])


@pytest.mark.parametrize("variant", ["w", "w_2"])
def test_forward_and_backward_run_the_grouped_head_kernels(variant):
    """ops.KERNEL_LOG: one grouped head launch per direction and none of the per-head dense launches; E_Blur keeps them."""
    from dge_amd import ops
    from dge_amd.encoder_variants import BlurBE

    def names(E, **kw):
        img = R.randn("ew.img", (2, 3, 64, 64), 81, 0.5).cuda()
        ops.KERNEL_LOG = []
        try:
            x, w = E(img, **kw)
            ((x * x).sum() + (w * w).sum()).backward()
            return [n for n, _ in ops.KERNEL_LOG]
        finally:
            ops.KERNEL_LOG = None
    log = names(_cls(variant)(startf=32, maxf=512, layer_count=5, compute_dtype="f32").cuda())
    assert log.count("dge_heads_rows_fwd") == 1 and log.count("dge_heads_rows_bwd") == 1, log
    assert not any(n in ("dge_linear", "dge_linear_t", "dge_dense_wgrad") for n in log), log
    ref = names(BlurBE(startf=32, maxf=512, layer_count=5, compute_dtype="f32").cuda())
    assert ref.count("dge_linear") == 10 and ref.count("dge_linear_t") == 10 and ref.count("dge_dense_wgrad") == 10, ref
    assert not any(n.startswith("dge_heads_rows") for n in ref)


def test_frozen_encoder_gets_the_same_image_gradient_from_one_head_launch():
    from dge_amd import ops
    E, _ = _encw("w_2", "f32")
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        grads = []
        for frozen in (False, True):
            for p in E.parameters():
                p.requires_grad_(not frozen)
                p.grad = None
            img = R.randn("ew.img", (2, 3, 64, 64), 81, 0.5).cuda().requires_grad_(True)
            x, w = E(img)
            ((x * R.randn("ew.gx", tuple(x.shape), 83).cuda()).sum() + (w * R.randn("ew.gw", tuple(w.shape), 84).cuda()).sum()).backward()
            grads.append(img.grad.clone())
            assert all(p.grad is None for p in E.parameters()) if frozen else E.decode_block[0].inver_mod2.weight.grad is not None
        assert torch.equal(grads[0], grads[1])
    finally:
        ops.set_deterministic(was)


# ----------------------------------------------------------------------------------------------------------------- steps
@pytest.mark.parametrize("variant", ["w", "w_2"])
def test_two_phase_w_step_matches_reference_run(variant):
    """Two iterations of 3.E_align_w.py / 2.E_align_w_2.py at reduced size: the image step, then the step on loss_w * 0.01; every
    generator noise tensor replayed.  Bounds of test_two_phase_z_step_matches_reference_run."""
    from dge_amd.e_align_w import EAlignWStep
    from tests.test_e_align_z_gpu import _step_models
    g = golden("step_w.npz" if variant == "w" else "step_w2.npz")
    Gs, Gm, LP = _step_models()
    E, _ = _encw(variant, "f32")
    init = {k: v.detach().clone() for k, v in E.state_dict().items()}
    st = EAlignWStep(Gs, Gm, E, LP, lr=0.0015, batch_size=2)
    nshapes = [tuple(int(v) for v in s if v) for s in g["noise_shapes"].tolist()]
    n_first = int(g["noise_split"][0])
    assert len(nshapes) == 20 and n_first == 10 and int(g["noise_split"][1]) == 0
    for it in range(2):
        z = R.randn(f"wstep.z{it}", (2, 512), 1)
        nz = [R.randn(f"wstep.it{it}.noise{i}", s, 1) for i, s in enumerate(nshapes)]
        r = st.step(it, z=z, gen_noises=(nz[:n_first], nz[n_first:]))
        assert relerr(r["w1"], g[f"it{it}_w1"]) < 1e-4
        errs = dict(w2=relerr(r["w2"], g[f"it{it}_w2"]), imgs2=relerr(r["imgs2"], g[f"it{it}_imgs2"]))
        got = [float(r["loss_imgs"]), float(r["loss_w"]), float(r["loss_mslv"])]
        ref_l = g[f"it{it}_losses"]
        lerr = max(abs(a - b) / abs(b) for a, b in zip(got, ref_l))
        sd_e = E.state_dict()
        perr = 0.0
        for key in g.files:
            if key.startswith(f"it{it}_after_phase2:"):
                perr = max(perr, _l2rel(sd_e[key.split(":", 1)[1]], g[key]))
            elif key.startswith(f"it{it}_after_phase2_head:"):
                perr = max(perr, _l2rel(sd_e[key.split(":", 1)[1]].flatten()[:4096], g[key]))
        cs = float(g[f"it{it}_param_checksum"])
        cerr = abs(R.checksum({k: v.cpu() for k, v in sd_e.items()}) - cs) / cs
        meas("step_w", variant=variant, it=it, losses=lerr, params=perr, checksum=cerr, **errs)
        assert errs["w2"] < 2e-3 and errs["imgs2"] < 3e-3, (it, errs)
        assert lerr < 3e-3, (it, got, ref_l)
        assert perr < 1.5e-3, (it, perr)
        assert cerr < 1e-5, (it, cerr)
    moved = [k for k in init if not torch.equal(init[k], E.state_dict()[k])]
    if variant == "w_2":
        for k in init:
            if "inver_mod1" in k:
                assert torch.equal(init[k], E.state_dict()[k]), k            # never a gradient, never an optimizer state
        assert not any("inver_mod1" in k for k in moved) and any("inver_mod2" in k for k in moved)
        assert all(len(st.opt.state.get(p, {})) == 0 for k, p in E.named_parameters() if "inver_mod1" in k)
    else:
        assert any("inver_mod1" in k for k in moved)


@pytest.mark.parametrize("variant", ["w", "w_2"])
def test_fullsize_bf16_w_step_runs_and_trains(variant):
    """One bf16 step at StyleGAN1 FFHQ-1024 (startf 16, 9 blocks, batch 2): finite losses, block 0 and the last block's inver_mod2 move."""
    from dge_amd.e_align_w import EAlignWStep, build_models_w
    Gs, Gm, E, LP = build_models_w(variant, 1024, 16, "bf16")
    assert type(E) is _cls(variant) and E.layer_count == 9
    st = EAlignWStep(Gs, Gm, E, LP, batch_size=2)
    keys = ("decode_block.8.inver_mod2.weight", "decode_block.0.conv_1.weight", "decode_block.0.inver_mod2.weight", "FromRGB.from_rgb.weight")
    before = {k: E.state_dict()[k].clone() for k in keys + ("decode_block.8.inver_mod1.weight",)}
    r = st.step(0)
    assert tuple(r["imgs2"].shape) == (2, 3, 1024, 1024) and tuple(r["w2"].shape) == (2, 18, 512)
    assert np.isfinite(float(r["loss_imgs"])) and np.isfinite(float(r["loss_w"])) and np.isfinite(float(r["loss_mslv"]))
    for k in keys:
        assert not torch.equal(E.state_dict()[k], before[k]), k
    same1 = torch.equal(E.state_dict()["decode_block.8.inver_mod1.weight"], before["decode_block.8.inver_mod1.weight"])
    assert same1 == (variant == "w_2")
