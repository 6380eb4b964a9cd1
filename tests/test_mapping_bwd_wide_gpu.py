"""dge_mapping_bwd_wide (ops.mapping_bwd(..., wide=True): the mapping adjoint as one chip-wide launch per layer) against the float64
restatement of tests/test_s2_mapping_fixture.py on the same operands, at the smallest shapes where its tiling can go wrong: batch
tile 8 (B = 9 is one more), 128-column / 32-row tiles (widths 12 and 36 are multiples of 4 but of no tile), 1 / 2 / 8 layers.
Bound: relerr <= 1e-5, the bound test_mapping_dz_vs_reference_golden applies to the same quantity."""
import numpy as np
import pytest
import torch

from tests.golden import recipe as R
from tests.test_s2_mapping_fixture import dense_layer, mapping_bwd_ref

pytestmark = pytest.mark.gpu
BATCH_TILE = 8          # kWideBT of csrc/mapping_kernels.hip


class Layer:
    """What ops._dense_layers reads (a DenseBlock's surface)."""

    def __init__(self, name, I, O, act, seed):
        self.weight = R.randn(name + ".w", (O, I), seed).cuda()
        self.bias = R.randn(name + ".b", (O,), seed, 0.3).cuda()
        self.wscale, self.bscale, self.additional_bias, self.act = 1.3 / float(np.sqrt(I)), 0.7, 0.05, act
        self.gain = float(np.sqrt(2.0)) if act == 1 else 1.0

    def ref(self):
        return dense_layer(self.weight.cpu().numpy(), self.bias.cpu().numpy(), self.wscale, self.bscale, self.additional_bias, self.act,
                           self.gain)


# (widths, activations): 1, 2 and 8 layers; 12 and 36 are multiples of 4 but of no tile; the 3-layer chain has an `act = none` layer inside
CHAINS = {
    "512-512": ((512, 512), (1,)),
    "64-128-512": ((64, 128, 512), (1, 1)),
    "12-512-36": ((12, 512, 36), (1, 1)),
    "12-512-36-64": ((12, 512, 36, 64), (1, 0, 1)),
    "8x512": ((512,) * 9, (1,) * 8),
}
_CHAIN_CACHE = {}


def make_chain(name):
    if name not in _CHAIN_CACHE:
        widths, acts = CHAINS[name]
        _CHAIN_CACHE[name] = [Layer(f"wide.{name}.{i}", widths[i], widths[i + 1], acts[i], 90 + i) for i in range(len(acts))]
    return _CHAIN_CACHE[name]


def forward(z, layers, pixelnorm):
    from dge_amd import ops
    x = ops.pixelnorm(z.contiguous()) if pixelnorm else z.contiguous()
    acts = []
    for Ly in layers:
        x = ops.linear(x, Ly.weight, Ly.bias, Ly.wscale, Ly.bscale, Ly.additional_bias, Ly.act, Ly.gain)
        acts.append(x)
    return acts


def relerr(a, b):
    return float(np.abs(a.detach().cpu().numpy().astype(np.float64) - b).max() / np.abs(b).max())


def run_wide(z, layers, g, coefs, acts, pixelnorm, **kw):
    from dge_amd import ops
    return ops.mapping_bwd(z, layers, g, coefs=coefs, acts=acts, pixelnorm=pixelnorm, wide=True, **kw)


@pytest.mark.parametrize("L,with_coefs,pixelnorm", [(1, False, True), (10, True, False), (18, True, True), (18, False, False)])
@pytest.mark.parametrize("B", [1, 3, BATCH_TILE + 1])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_wide_adjoint_matches_float64_restatement(chain, B, L, with_coefs, pixelnorm):
    from dge_amd import ops
    layers = make_chain(chain)
    I0, D = layers[0].weight.shape[1], layers[-1].weight.shape[0]
    z = R.randn(f"wide.z.{chain}", (B, I0), 7).cuda()
    g = R.randn(f"wide.g.{chain}.{L}", (B, L, D), 8).cuda()
    coefs = (R.randn(f"wide.c.{L}", (L,), 9).abs() + 0.2).cuda() if with_coefs else None
    acts = forward(z, layers, pixelnorm)
    work = torch.full((ops.mapping_bwd_work_bytes(B) // 4,), float("nan"), device="cuda").view(torch.uint8)
    dz = run_wide(z, layers, g, coefs, acts, pixelnorm, work=work)
    assert torch.isfinite(dz).all()          # every workspace element the launches read was written by them (nothing pre-zeroed)
    ref = mapping_bwd_ref(z.cpu().numpy(), [Ly.ref() for Ly in layers], g.cpu().numpy(), None if coefs is None else coefs.cpu().numpy(),
                          acts=[a.cpu().numpy() for a in acts], pixelnorm=pixelnorm)
    e = relerr(dz, ref)
    one = ops.mapping_bwd(z, layers, g, coefs=coefs, acts=acts, pixelnorm=pixelnorm)
    e1 = relerr(dz, one.cpu().numpy().astype(np.float64))
    print(f"MEAS mapping_bwd_wide {chain} B={B} L={L} coefs={with_coefs} pn={pixelnorm}: vs f64 {e:.3e}, vs dge_mapping_bwd {e1:.3e}, "
          f"bit-equal {torch.equal(dz, one)}")
    assert e <= 1e-5, e
    assert e1 <= 1e-5, e1
    # the same bits on a second call, in the other reduction mode, and for a row run alone
    assert torch.equal(dz, run_wide(z, layers, g, coefs, acts, pixelnorm))
    was = ops.is_deterministic()
    ops.set_deterministic(not was)
    try:
        assert torch.equal(dz, run_wide(z, layers, g, coefs, acts, pixelnorm))
    finally:
        ops.set_deterministic(was)
    for b in sorted({0, B - 1}):
        alone = run_wide(z[b:b + 1], layers, g[b:b + 1], coefs, [a[b:b + 1].contiguous() for a in acts], pixelnorm)
        assert torch.equal(alone[0], dz[b]), b


def test_wide_adjoint_row_strides_and_zero_activations():
    """ldz / lddz larger than the width, and saved activations with entries exactly 0: the slope there is dge_mapping_bwd's (the
    negative side: 0.2 for leaky-relu), so the two kernels agree and both match the restatement."""
    from dge_amd import ops
    layers = make_chain("64-128-512")
    B, L = 3, 10
    zbig = R.randn("wide.zs", (B, 96), 7).cuda()
    z = zbig[:, :64]
    g = R.randn("wide.gs", (B, L, 512), 8).cuda()
    acts = forward(z.contiguous(), layers, True)
    acts[0][:, ::3] = 0.0
    acts[1][:, 1::2] = 0.0
    out_big = torch.full((B, 80), 7.0, device="cuda")
    dz = run_wide(z, layers, g, None, acts, True, out=out_big[:, :64])
    assert dz.stride(0) == 80 and torch.all(out_big[:, 64:] == 7.0)
    ref = mapping_bwd_ref(z.cpu().numpy(), [Ly.ref() for Ly in layers], g.cpu().numpy(), None, acts=[a.cpu().numpy() for a in acts])
    assert relerr(dz, ref) <= 1e-5
    one = ops.mapping_bwd(z.contiguous(), layers, g, acts=acts)
    assert relerr(dz, one.cpu().numpy().astype(np.float64)) <= 1e-5
    assert torch.equal(dz, run_wide(z.contiguous(), layers, g, None, acts, True))


def test_wide_adjoint_is_logged_and_needs_saved_activations():
    from dge_amd import ops
    layers = make_chain("512-512")
    z = R.randn("wide.z.512-512", (1, 512), 7).cuda()
    g = R.randn("wide.g.512-512.1", (1, 1, 512), 8).cuda()
    acts = forward(z, layers, True)
    log = []
    ops.KERNEL_LOG = log
    try:
        run_wide(z, layers, g, None, acts, True)
        ops.mapping_bwd(z, layers, g, acts=acts)          # (the one-launch form logs what it logged: nothing)
    finally:
        ops.KERNEL_LOG = None
    assert [n for n, _ in log] == ["dge_mapping_bwd_wide"]
    with pytest.raises(ops.DgeError, match="acts"):
        run_wide(z, layers, g, None, None, True)
    with pytest.raises(ops.DgeError, match="work"):
        run_wide(z, layers, g, None, acts, True, work=torch.empty(16, dtype=torch.uint8, device="cuda"))
