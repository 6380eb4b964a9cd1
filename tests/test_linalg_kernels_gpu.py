"""The kernels of csrc/linalg_kernels.hip at the smallest shapes where each can go wrong: dge_gram against float64 on the same f32
operands within a derived bound, dge_eigh_sym against numpy.linalg.eigh in float64 on the same f32 matrix within tau(A) = 3 x the
error of the plain f32 Jacobi restatement (tests/directions_ref.py).  Both give the same bits from run to run, dge_gram also in
both reduction modes."""
import numpy as np
import pytest
import torch

from tests import directions_ref as DR
from tests.conftest import meas
from tests.golden import recipe as R

pytestmark = pytest.mark.gpu


def both_modes(fn):
    """fn() in the default and in the deterministic reduction mode (twice): the same bits -> the result"""
    from dge_amd import ops
    was = ops.is_deterministic()
    outs = []
    try:
        for on in (False, True, True):
            ops.set_deterministic(on)
            outs.append(fn().clone())
    finally:
        ops.set_deterministic(was)
    for o in outs[1:]:
        assert torch.equal(outs[0], o)
    return outs[0]


# ------------------------------------------------------------------ dge_gram
GRAM_SHAPES = [(1, 1), (3, 5), (7, 33), (65, 64), (1025, 130), (300, 512)]


@pytest.mark.parametrize("N,D", GRAM_SHAPES)
def test_gram_against_float64(N, D):
    """Per element: |out - ref| <= (N + 16) 2^-24 sum_n |u_ni u_nj| - N roundings of the f32 accumulation at the most, the rounding
    of x - mean in each factor, the chunk sums and the scale; with row_norm (N + D + 16): the f32 norm of a row carries up to D / 2
    roundings into each factor.  One row is zero wherever there is more than one; every variant also runs on a view with a row
    stride above D."""
    from dge_amd import ops
    x = R.randn(f"linalg.gram.{N}x{D}", (N, D + 5), 31)
    if N > 1:
        x[1] = 0.0
    wide = x.cuda()
    worst = {}
    for view in (False, True):
        xd = wide[:, 3:3 + D] if view else wide[:, 3:3 + D].contiguous()
        assert (xd.stride(0) > D) == view or N == 1
        xh = x[:, 3:3 + D].numpy()
        mean = torch.from_numpy(xh.mean(axis=0, dtype=np.float32))
        for tag, kw, scale in (("plain", {}, 0.37), ("mean", dict(mean=mean), 1.0 / N), ("row_norm", dict(row_norm=True), 1.0)):
            dkw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
            out = both_modes(lambda: ops.gram(xd, scale=scale, **dkw))
            assert ops.last_kernel() == "gram"
            assert torch.equal(out, out.t()), tag                                    # one triangle computed, the other its mirror
            assert torch.equal(ops.gram(xd, scale=scale, **dkw), out), tag            # a second call: the same bits
            ref, bound = DR.gram_ref(xh, mean=None if "mean" not in kw else mean.numpy(), row_norm="row_norm" in kw,
                                     scale=float(np.float32(scale)))
            err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
            assert tuple(out.shape) == (D, D) and np.all(err <= bound), (tag, view, float((err - bound).max()))
            worst[tag] = max(worst.get(tag, 0.0), float((err / np.maximum(bound, 1e-300)).max()))
        if N > 1:          # a zero row contributes nothing: row 1 above inside the bound (no 0 / 0), one appended to the bit
            keep = torch.cat((xd[:1], xd[2:])).contiguous()
            more = torch.cat((keep, torch.zeros(1, D, device="cuda")))
            assert torch.equal(ops.gram(more, row_norm=True), ops.gram(keep, row_norm=True))
    meas(f"linalg.gram.{N}x{D}", **{f"{k}_of_bound": v for k, v in worst.items()})


def test_gram_refusals():
    from dge_amd import ops
    from dge_amd._lib import DgeError
    x = torch.ones(4, 8, device="cuda")
    for bad, kw in ((torch.ones(4, 1025, device="cuda"), {}), (torch.ones(0, 8, device="cuda"), {}), (torch.ones(4, 0, device="cuda"), {}),
                    (x, dict(row_norm=True, mean=torch.zeros(8, device="cuda"))), (x, dict(mean=torch.zeros(7, device="cuda"))),
                    (x.double(), {}), (x.t(), {}), (x.cpu(), {}), (torch.ones(8, device="cuda"), {})):
        with pytest.raises(DgeError):
            ops.gram(bad, **kw)
    lib = ops.lib()
    assert lib.dge_gram_work_bytes(0, 8) == -1 and lib.dge_gram_work_bytes(4, 1025) == -1 and lib.dge_gram_work_bytes(4, 0) == -1
    assert lib.dge_gram_work_bytes(1 << 40, 8) == -1
    nb = lib.dge_gram_work_bytes(4, 8)
    work, out = torch.empty(nb // 4, device="cuda"), torch.full((8, 8), 7.0, device="cuda")
    P = lambda t: ops._p(t)
    st = ops._stream()
    assert lib.dge_gram(P(x), 4, 8, 7, None, 0, 1.0, P(out), P(work), nb, st) == -1           # a row stride below D
    assert lib.dge_gram(P(x), 4, 8, 8, None, 0, 1.0, P(out), P(work), nb - 4, st) == -1       # a workspace too small
    assert lib.dge_gram(P(x), 4, 8, 8, None, 0, 1.0, None, P(work), nb, st) == -1
    assert b"gram" in lib.dge_last_error()
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)                                                     # a refused call touches nothing
    assert torch.equal(ops.gram(x), torch.full((8, 8), 4.0, device="cuda"))


# ------------------------------------------------------------------ dge_eigh_sym
def unit_err(x, A2):
    return float(x) / (DR.U * A2)


@pytest.mark.parametrize("name", list(DR.MATRICES))
def test_eigh_sym_against_float64(name):
    from dge_amd import ops
    A, lam, V, tau, ref_err = DR.matrix(name)
    kind = DR.MATRICES[name][1]
    D = A.shape[0]
    A2 = float(np.abs(lam).max())
    a = torch.from_numpy(A.copy()).cuda()          # (the shared array is read-only)
    evals, evecs, (sweeps, off) = ops.eigh_sym(a)
    assert ops.last_kernel() == "eigh_sym"
    e2, v2, st2 = ops.eigh_sym(a)
    assert torch.equal(e2, evals) and torch.equal(v2, evecs) and st2 == (sweeps, off)          # a second call: the same bits
    low = torch.triu(a) + torch.tril(torch.full_like(a, float("nan")), -1)                   # only the upper triangle is read
    e3, v3, _ = ops.eigh_sym(low)
    assert torch.equal(e3, evals) and torch.equal(v3, evecs)
    ev, Vh = evals.cpu().numpy().astype(np.float64), evecs.cpu().numpy().astype(np.float64)
    A64 = A.astype(np.float64)
    m = dict(tau=unit_err(tau, A2), restatement=unit_err(ref_err, A2), sweeps=sweeps, off=off)
    m["evals"] = unit_err(np.abs(ev - lam).max(), A2)
    m["orth"] = unit_err(np.abs(Vh @ Vh.T - np.eye(D)).max() * A2, A2)
    m["residual"] = unit_err(np.abs(Vh @ A64 - ev[:, None] * Vh).max(), A2)
    if kind != "values":
        bounds, cluster = DR.vector_bounds(name)
        Vn = Vh / np.linalg.norm(Vh, axis=1, keepdims=True)
        sin = np.linalg.norm(Vn - np.sum(Vn * V, axis=1, keepdims=True) * V, axis=1)
        simple = np.isfinite(bounds)
        m["sin_of_bound"] = float((sin[simple] / bounds[simple]).max())
        if cluster is not None:
            m["cluster_of_bound"] = float(np.linalg.norm(Vn[DR.CLUSTER].T @ Vn[DR.CLUSTER] - V[DR.CLUSTER].T @ V[DR.CLUSTER], 2) / cluster)
    meas(f"linalg.eigh_sym.{name}", **m)
    assert np.abs(ev - lam).max() <= tau, m
    assert np.abs(Vh @ Vh.T - np.eye(D)).max() <= tau / A2, m
    assert np.abs(Vh @ A64 - ev[:, None] * Vh).max() <= tau, m
    assert np.all(np.diff(ev) <= 0), "descending order"
    top = np.argmax(np.abs(Vh), axis=1)                                                      # the first of equal maxima
    assert np.all(Vh[np.arange(D), top] > 0), "sign rule"
    fro = float(np.linalg.norm(A64))
    assert (1 if D > 1 else 0) <= sweeps <= 30 and 0.0 <= off <= 2.0 ** -40 * fro * (1 + 1e-6), (sweeps, off)
    if kind != "values":
        assert m["sin_of_bound"] <= 1.0, m
        if cluster is not None:
            assert m["cluster_of_bound"] <= 1.0, m


def test_eigh_sym_diagonal_and_identity():
    """Nothing to rotate: zero sweeps, the diagonal sorted, unit vectors with a positive entry; equal eigenvalues keep index order."""
    from dge_amd import ops
    d = torch.tensor([1.0, -2.0, 3.0, 3.0, 0.5])
    evals, evecs, (sweeps, off) = ops.eigh_sym(torch.diag(d).cuda())
    assert sweeps == 0 and off == 0.0
    assert evals.cpu().tolist() == [3.0, 3.0, 1.0, 0.5, -2.0]
    assert torch.equal(evecs.cpu(), torch.eye(5)[[2, 3, 0, 4, 1]])


def test_eigh_sym_refusals_and_sweep_limit():
    from dge_amd import ops
    from dge_amd._lib import DgeError
    for bad in (torch.ones(1025, 1025, device="cuda"), torch.ones(0, 0, device="cuda"), torch.ones(3, 4, device="cuda"),
                torch.ones(4, 4, device="cuda").double(), torch.ones(4, 4)):
        with pytest.raises(DgeError):
            ops.eigh_sym(bad)
    a = torch.from_numpy(DR.matrix("d64")[0].copy()).cuda()
    for sweeps in (0, 1001):
        with pytest.raises(DgeError, match="max_sweeps"):
            ops.eigh_sym(a, max_sweeps=sweeps)
    assert ops.lib().dge_eigh_sym_work_bytes(1025) == -1 and ops.lib().dge_eigh_sym_work_bytes(0) == -1
    # one sweep does not diagonalise a dense 64 x 64 matrix: an error with a message, and the last iterate is written
    with pytest.raises(DgeError, match="not converged after 1 sweeps") as e:
        ops.eigh_sym(a, max_sweeps=1)
    evals, evecs, (sweeps, off) = e.value.partial
    lam = DR.matrix("d64")[1]
    assert sweeps == 1 and 0.0 < off < float(np.linalg.norm(DR.matrix("d64")[0]))
    # the sorted diagonal of an orthogonally similar matrix is within off(A) of the spectrum (Hoffman-Wielandt)
    assert torch.isfinite(evecs).all() and np.abs(evals.cpu().numpy() - lam).max() <= off + 1e-5
