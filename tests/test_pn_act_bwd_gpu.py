"""dge_pixelnorm_act_bwd (ops.pixelnorm_act_bwd): the pixel-norm backward of the PGGAN generator fused with the nearest-upsample
adjoint in front of it and the leaky-relu backward behind it, against a float64 restatement and against the three composed
launches (nearest_up2_bwd -> pixelnorm_nhwc_bwd -> act_bwd) on the same operands."""
import pytest
import torch

from tests.conftest import meas
from tests.golden import recipe as R

pytestmark = pytest.mark.gpu

EPS = 1e-8
_SIZES = [(3, 3), (4, 5), (8, 8)]
# the smallest channel count of the channel rule per dtype (one 16-byte chunk), 16, 64, 512 and, for bf16, the largest (128 chunks)
_CHANNELS = {"f32": [4, 16, 64, 512], "bf16": [8, 16, 64, 512, 1024]}


def _operands(cd, B, H, W, Cc, up):
    """g and x in the compute dtype; about one entry of x in eight is exactly 0 (and stays 0 in bf16)."""
    dt = torch.float32 if cd == "f32" else torch.bfloat16
    x = R.randn(f"pab.x.{H}.{W}.{Cc}", (B, H, W, Cc), 91)
    zero = R.randn(f"pab.zero.{H}.{W}.{Cc}", (B, H, W, Cc), 92) > 1.15
    x = torch.where(zero, torch.zeros(()), x).to(dt)
    gs = (B, 2 * H, 2 * W, Cc) if up else (B, H, W, Cc)
    g = R.randn(f"pab.g.{H}.{W}.{Cc}.{int(up)}", gs, 93).to(dt)
    assert int((x == 0).sum()) > 0
    return g.cuda(), x.cuda()


def _ref64(g, x, up, act):
    """gl = 2x2 block sum of g (up) or g; gx = r*gl - x*(sum_c gl*x)*r^3/C, r = rsqrt(mean_c x^2 + eps); out = gx * lrelu'(x) with
    lrelu'(x) = 1 for x > 0 and 0.2 otherwise (dge_act_bwd's rule at 0)."""
    g, x = g.double(), x.double()
    B, H, W, Cc = x.shape
    gl = g.view(B, H, 2, W, 2, Cc).sum(dim=(2, 4)) if up else g
    r = torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + EPS)
    gx = r * gl - x * (gl * x).sum(dim=-1, keepdim=True) * r ** 3 / Cc
    return gx * torch.where(x > 0, 1.0, 0.2) if act else gx


def _composed(g, x, up, act):
    from dge_amd import ops
    if up:
        g, _ = ops.nearest_up2_bwd(g)
    gx = ops.pixelnorm_nhwc_bwd(g, x, EPS)
    return ops.act_bwd(gx, x, None, pool=False, scale=1.0) if act else gx


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("HW", _SIZES)
def test_f32_against_float64_and_the_activation_rule_at_zero(HW, up, act):
    """f32: within 1e-6 of the largest element of the float64 restatement (a few f32 ulps of it: the bound
    test_case2_gpu sets for a kernel whose expression the compiler may contract differently), for every channel count; the entries
    where x == 0 equal dge_act_bwd's result on the un-activated gradient to the bit.  2 * H * W pixels never fill the last
    workgroup's pixel slots at C <= 64 (64, 16 and 4 pixels per wave), and 2 * 3 * 3 = 18 leaves a ragged wave at C = 512."""
    from dge_amd import ops
    H, W = HW
    for Cc in _CHANNELS["f32"]:
        assert ops.pixelnorm_act_bwd_supported(Cc, ops.F32)
        g, x = _operands("f32", 2, H, W, Cc, up)
        ops.KERNEL_LOG = log = []
        try:
            out = ops.pixelnorm_act_bwd(g, x, up=up, act=act, eps=EPS)
        finally:
            ops.KERNEL_LOG = None
        assert [n for n, _ in log] == [f"pixelnorm_act_bwd<f32,{'up' if up else 'same'},{'act' if act else 'lin'}>"], log
        ref = _ref64(g, x, up, act)
        err = ((out.double() - ref).abs().max() / ref.abs().max()).item()
        meas("pn_act_bwd_f32", H=H, W=W, C=Cc, up=float(up), act=float(act), err=err)
        assert err <= 1e-6, (Cc, err)
        if act:
            lin = ops.pixelnorm_act_bwd(g, x, up=up, act=False, eps=EPS)
            via_act_bwd = ops.act_bwd(lin, x, None, pool=False, scale=1.0, slope=0.2)
            at0 = x == 0
            assert torch.equal(out[at0], via_act_bwd[at0]), Cc


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("HW", _SIZES)
def test_bf16_is_no_worse_than_the_composed_launches(HW, up, act):
    """bf16: the distance (L2 over the tensor) to the float64 restatement on the same bf16 operands is no larger than that of
    nearest_up2_bwd -> pixelnorm_nhwc_bwd -> act_bwd, which round the gradient to bf16 after every launch."""
    from dge_amd import ops
    H, W = HW
    for Cc in _CHANNELS["bf16"]:
        assert ops.pixelnorm_act_bwd_supported(Cc, ops.BF16)
        g, x = _operands("bf16", 2, H, W, Cc, up)
        out = ops.pixelnorm_act_bwd(g, x, up=up, act=act, eps=EPS)
        assert out.dtype == torch.bfloat16 and out.shape == x.shape
        ref = _ref64(g, x, up, act)
        e_fused = (out.double() - ref).norm().item() / ref.norm().item()
        e_comp = (_composed(g, x, up, act).double() - ref).norm().item() / ref.norm().item()
        meas("pn_act_bwd_bf16", H=H, W=W, C=Cc, up=float(up), act=float(act), fused=e_fused, composed=e_comp)
        assert e_fused <= e_comp, (Cc, e_fused, e_comp)
        assert e_fused < 4e-3, (Cc, e_fused)          # one bf16 rounding: 2^-9 per element at the most


def test_same_bits_in_both_reduction_modes():
    from dge_amd import ops
    g, x = _operands("bf16", 2, 4, 5, 64, True)
    was = ops.is_deterministic()
    outs = []
    try:
        for det in (True, False):
            ops.set_deterministic(det)
            outs.append(ops.pixelnorm_act_bwd(g, x, up=True))
    finally:
        ops.set_deterministic(was)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("cd,Cc", [("f32", 6), ("f32", 12), ("f32", 1024), ("bf16", 4), ("bf16", 24), ("bf16", 2048)])
def test_unsupported_channel_count_is_an_error(cd, Cc):
    """No multiple of a 16-byte chunk, no power-of-two number of chunks, more than two chunks per lane: an error string, no launch."""
    from dge_amd import ops
    dt = torch.float32 if cd == "f32" else torch.bfloat16
    assert not ops.pixelnorm_act_bwd_supported(Cc, ops.F32 if cd == "f32" else ops.BF16)
    x = torch.ones((1, 2, 2, Cc), dtype=dt, device="cuda")
    with pytest.raises(ops.DgeError, match="pixelnorm_act_bwd"):
        ops.pixelnorm_act_bwd(torch.ones_like(x), x)
    torch.cuda.synchronize()


def test_operand_shapes_are_checked():
    from dge_amd import ops
    x = torch.ones((1, 2, 2, 16), dtype=torch.float32, device="cuda")
    with pytest.raises(ops.DgeError, match="does not go with"):
        ops.pixelnorm_act_bwd(x, x, up=True)
