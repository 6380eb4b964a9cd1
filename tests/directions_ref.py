"""What the direction tests share: float64 restatements of SeFa and of the W-space PCA on numpy.linalg.eigh, the plain f32 Jacobi
restatement whose own error sets the eigenvalue tolerance, and the constructors of the test matrices."""
import functools

import numpy as np

U = 2.0 ** -24          # the unit roundoff of f32


# ------------------------------------------------------------------ float64 restatements
def sign_rule(V):
    """Rows of V with their component of largest magnitude positive (ties: the lowest index)."""
    V = np.array(V, copy=True)
    for k in range(V.shape[0]):
        j = int(np.argmax(np.abs(V[k])))          # argmax returns the first of equal maxima
        if V[k, j] < 0:
            V[k] = -V[k]
    return V


def eigh_ref(A):
    """A (any float dtype, symmetric) -> (evals descending [D], evecs [D,D] with the eigenvector of evals[k] in row k, sign rule
    applied), float64, numpy.linalg.eigh on the upper triangle."""
    lam, Q = np.linalg.eigh(np.asarray(A, dtype=np.float64), UPLO="U")
    return lam[::-1].copy(), sign_rule(Q.T[::-1])


def sefa_matrix_ref(weights):
    """weights: the style weight matrices [C_g,512] of the chosen blocks in block order -> M = sum of the outer products of the
    unit rows, float64 (a zero row contributes nothing)."""
    A = np.concatenate([np.asarray(w, dtype=np.float64) for w in weights])
    n = np.linalg.norm(A, axis=1, keepdims=True)
    A = np.divide(A, n, out=np.zeros_like(A), where=n > 0)
    return A.T @ A


def pca_matrix_ref(w, mean):
    """w [N,D] and mean [D] as the device holds them (f32) -> the covariance sum (w - mean)(w - mean)^T / N in float64."""
    d = np.asarray(w, dtype=np.float64) - np.asarray(mean, dtype=np.float64)
    return d.T @ d / w.shape[0]


def gram_ref(x, mean=None, row_norm=False, scale=1.0):
    """(out, bound) of dge_gram in float64 on the same f32 operands: bound[i,j] = (N + 16) 2^-24 sum_n |u_ni u_nj| (|scale| folded in),
    with row_norm (N + D + 16) 2^-24 ..."""
    u = np.asarray(x, dtype=np.float64)
    N, D = u.shape
    k = N + 16
    if row_norm:
        n = np.linalg.norm(u, axis=1, keepdims=True)
        u = np.divide(u, n, out=np.zeros_like(u), where=n > 0)
        k += D
    if mean is not None:
        u = u - np.asarray(mean, dtype=np.float64)
    return scale * (u.T @ u), abs(scale) * k * U * (np.abs(u).T @ np.abs(u))


# ------------------------------------------------------------------ the f32 Jacobi restatement
def round_robin(D):
    """The rounds of the round-robin schedule on D indices: a list of index arrays (p, q, rest) with p < q, every pair once a
    sweep; `rest` holds the index that sits a round out (odd D: the bye)."""
    n = D + (D & 1)
    m = n - 1
    rounds = []
    for r in range(m):
        a = [m] + [(r + k) % m for k in range(1, n // 2)]
        b = [r] + [(r - k) % m for k in range(1, n // 2)]
        pairs = [(min(x, y), max(x, y)) for x, y in zip(a, b) if x < D and y < D]
        rest = sorted(set(range(D)) - {i for pq in pairs for i in pq})
        if pairs:
            rounds.append((np.array([p for p, _ in pairs]), np.array([q for _, q in pairs]), np.array(rest, dtype=np.int64)))
    return rounds


def _rows_numpy(A, p, q, rest, c, s):
    """J^T A for the disjoint rotations (p, q, c, s): row p <- c row p - s row q, row q <- s row p + c row q (f32, each operation
    rounded once)"""
    B = np.empty_like(A)
    rp, rq = A[p], A[q]
    B[p] = c[:, None] * rp - s[:, None] * rq
    B[q] = s[:, None] * rp + c[:, None] * rq
    B[rest] = A[rest]
    return B


def _rows_torch(A, p, q, rest, c, s):
    """_rows_numpy on CPU torch tensors over the same memory: the same IEEE f32 operations in the same order, several times as fast
    at D = 512 (tests/test_directions_cpu.py holds the two to equal bits)"""
    import torch
    At = torch.from_numpy(A)
    pt, qt, ct, st = torch.from_numpy(p), torch.from_numpy(q), torch.from_numpy(c)[:, None], torch.from_numpy(s)[:, None]
    rp, rq = At.index_select(0, pt), At.index_select(0, qt)
    B = torch.empty_like(At)
    B.index_copy_(0, pt, ct * rp - st * rq)
    B.index_copy_(0, qt, st * rp + ct * rq)
    if len(rest):
        B[torch.from_numpy(rest)] = At[torch.from_numpy(rest)]
    return B.numpy()


def jacobi_f32(A, max_sweeps=60, backend="torch"):
    """Cyclic two-sided Jacobi in float32, round-robin order: t = sign(theta) / (|theta| + sqrt(1 + theta^2)) with
    theta = (a_qq - a_pp) / (2 a_pq), c = 1 / sqrt(1 + t^2), s = t c (numpy float32; a_pq = 0: no rotation).  The disjoint rotations
    of a round are applied together (they commute), the two-sided update of the symmetric matrix as J^T (J^T A)^T, and the rotated
    pair's element is set to 0.  Stops when off(A) <= 2^-24 |A|_F.  backend: "numpy", or "torch" for the row updates (the same
    bits).  Returns (evals descending, sweeps)."""
    rows = {"numpy": _rows_numpy, "torch": _rows_torch}[backend]
    A = np.array(A, dtype=np.float32, copy=True)
    D = A.shape[0]
    one = np.float32(1)
    fro = float(np.sqrt(np.sum(A.astype(np.float64) ** 2)))
    rounds = round_robin(D)
    sweeps = 0

    def off(M):
        M = M.astype(np.float64)
        return np.sqrt(max(float(np.sum(M * M) - np.sum(np.diag(M) ** 2)), 0.0))
    while off(A) > U * fro and sweeps < max_sweeps:
        for p, q, rest in rounds:
            apq = A[p, q]
            with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
                theta = (A[q, q] - A[p, p]) / (np.float32(2) * apq)
                t = np.where(theta >= 0, one, -one) / (np.abs(theta) + np.sqrt(one + theta * theta))
            t = np.where(apq != 0, t, np.float32(0)).astype(np.float32)
            c = (one / np.sqrt(one + t * t)).astype(np.float32)
            s = (t * c).astype(np.float32)
            A = rows(np.ascontiguousarray(rows(A, p, q, rest, c, s).T), p, q, rest, c, s)
            A[p, q] = A[q, p] = 0          # the element the rotation annihilates
        sweeps += 1
    return np.sort(np.diag(A).astype(np.float64))[::-1].copy(), sweeps


def eig_tolerance(A):
    """tau(A): 3 x the largest eigenvalue error of the f32 Jacobi restatement on A against numpy.linalg.eigh in float64 on the same
    matrix.  The factor 3 covers another rotation order and another summation order.  Returns (tau, the restatement's error)."""
    lam, _ = eigh_ref(A)
    got, _ = jacobi_f32(A)
    err = float(np.abs(got - lam).max())
    return 3.0 * err, err


# ------------------------------------------------------------------ the test matrices
def _sym32(A):
    A = np.asarray(A, dtype=np.float64).astype(np.float32)
    return np.triu(A) + np.triu(A, 1).T


def _with_spectrum(lam, seed):
    D = len(lam)
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((D, D)))
    return _sym32((Q * np.asarray(lam, dtype=np.float64)) @ Q.T)


def _cluster33():
    lam = np.linspace(3, 1, 33)
    lam[4:8] = 2.5
    return lam


# name -> (constructor, kind): "simple" = every eigenvalue simple and separated (every vector is checked), "cluster" = the D = 33
# matrix with its fourfold eigenvalue (the eigenspace as a projector, the simple ones as vectors), "values" = no controlled gaps
# (eigenvalues, orthogonality and residuals only)
MATRICES = {
    "d1": (lambda: np.array([[3.0]], dtype=np.float32), "values"),
    "d2": (lambda: _with_spectrum(np.linspace(3, 1, 2), 102), "simple"),
    "d5": (lambda: _with_spectrum(np.linspace(3, 1, 5), 105), "simple"),
    "d33_cluster": (lambda: _with_spectrum(_cluster33(), 133), "cluster"),
    "d64": (lambda: _with_spectrum(np.linspace(3, 1, 64), 164), "simple"),
    "d64_indefinite": (lambda: _with_spectrum(np.linspace(2, -1, 64), 165), "simple"),
    "d64_rank32": (lambda: _gram_of(np.random.default_rng(166).standard_normal((32, 64))), "values"),
    "d128_geom": (lambda: _with_spectrum(np.geomspace(1, 1e-4, 128), 228), "simple"),
    "d512_gram": (lambda: _gram_of(_unit_rows(np.random.default_rng(612).standard_normal((2048, 512)))), "values"),
}
# The positions of the repeated eigenvalue of d33_cluster in descending order.  linspace(3, 1, 33) steps by 1/16, so its element 8 is
# 2.5 already: setting lam[4:8] = 2.5 makes the eigenvalue fivefold (positions 4 .. 8), and the eigenspace that is compared as a
# projector has five dimensions.
CLUSTER = slice(4, 9)
# The bound of a vector check is tau / gap, and never above this: where tau / gap is larger (d128_geom: the spectrum is geometric down
# to 1e-4, its smallest gaps are 7.5e-6, and tau, an absolute error, is about 6e-5) the check would hold for any unit vector.
# Capping the bound keeps every vector checked and no check vacuous.
VECTOR_CAP = 0.05


def vector_bounds(name):
    """(bounds [D] on sin angle(v^_k, v_k) for the simple eigenvalues - inf at the members of the cluster -, the bound of the
    cluster's projector or None): min(tau / gap, VECTOR_CAP)."""
    _, lam, _, tau, _ = matrix(name)
    kind = MATRICES[name][1]
    assert kind in ("simple", "cluster")
    b = np.minimum(tau / gaps(lam), VECTOR_CAP)
    if kind == "simple":
        return b, None
    b[CLUSTER] = np.inf
    return b, min(tau / gaps(lam, CLUSTER), VECTOR_CAP)


def _unit_rows(X):
    return X / np.linalg.norm(X, axis=1, keepdims=True)


def _gram_of(X):
    return _sym32(X.T @ X)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(A f32 symmetric, evals float64 descending, evecs float64 rows, tau, the restatement's error): built once per process and
    shared; the arrays are read-only."""
    A = MATRICES[name][0]()
    lam, V = eigh_ref(A)
    tau, err = eig_tolerance(A)
    for x in (A, lam, V):
        x.setflags(write=False)
    return A, lam, V, tau, err


def gaps(lam, members=None):
    """gap_k = the distance of lam[k] to the nearest other eigenvalue; with `members` (a slice): the distance of the cluster to the
    nearest eigenvalue outside it."""
    lam = np.asarray(lam, dtype=np.float64)
    if members is not None:
        inside = np.zeros(len(lam), dtype=bool)
        inside[members] = True
        return float(np.abs(lam[inside][:, None] - lam[~inside][None, :]).min())
    d = np.abs(lam[:, None] - lam[None, :])
    np.fill_diagonal(d, np.inf)
    return d.min(axis=1)
