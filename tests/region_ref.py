"""A numpy float64 restatement of the region-direction solve (dge_amd.region_directions.solve_region and the direction step), of the
weighted Gram matrices with dge_gram_cols' error bound, and of what the tests measure on the results."""
import numpy as np

from tests.directions_ref import U, eigh_ref, sign_rule


def pooled_weights(mask, s):
    """mask [H,W] -> the s x s area means, flattened [(H/s) (W/s)], float64"""
    m = np.asarray(mask, dtype=np.float64)
    H, W = m.shape
    return m.reshape(H // s, s, W // s, s).mean(axis=(1, 3)).reshape(-1)


def grams_ref(X, mu):
    """X [K,N], mu [P] with P dividing N -> (M_f, M_b) in float64: column n has weight mu[n mod P]"""
    X = np.asarray(X, dtype=np.float64)
    w = np.tile(np.asarray(mu, dtype=np.float64), X.shape[1] // len(mu))
    return (X * w) @ X.T, (X * (1.0 - w)) @ X.T


def gram_cols_ref(x, wgt, chunk, scale=1.0):
    """(out_a, out_b, bound_a, bound_b) of dge_gram_cols in float64 on the same f32 operands (wgt None: w = 1, out_b / bound_b None).
    bound = (c + n_c + 16) 2^-24 |scale| sum_n |w_n x_in x_jn| with c the columns of a chunk and n_c the chunks: an element's chunk sum
    carries at most c roundings of its f32 accumulation, the chunk sums are added with n_c more, and the 16 cover the rounding of
    w_n x_jn (and of 1.0f - w_n) in the operand, the scale and the result."""
    x = np.asarray(x, dtype=np.float64)
    K, N = x.shape
    nc = -(-N // chunk)
    k = (min(chunk, N) + nc + 16) * U * abs(scale)
    ax = np.abs(x)
    if wgt is None:
        return scale * (x @ x.T), None, k * (ax @ ax.T), None
    w32 = np.asarray(wgt, dtype=np.float32)
    w = np.tile(w32.astype(np.float64), N // len(w32))
    wb = np.tile((np.float32(1.0) - w32).astype(np.float64), N // len(w32))          # 1.0f - w as the kernel forms it
    return scale * ((x * w) @ x.T), scale * ((x * wb) @ x.T), k * ((ax * np.abs(w)) @ ax.T), k * ((ax * np.abs(wb)) @ ax.T)


def region_eps(M_f, M_b, reg):
    K = M_b.shape[0]
    tb, tf = float(np.trace(M_b)), float(np.trace(M_f))
    if tb == 0.0 and tf == 0.0:
        raise ValueError("both traces are 0")
    return reg * (tb if tb != 0.0 else tf) / K


def solve_ref(M_f, M_b, reg, Q=None):
    """(eps, ratio [K] descending, coeffs [K,K] unit rows, directions [K,D] or None): eps = reg tr(M_b) / K; (beta, U) = eigh(M_b);
    S = diag((max(beta, 0) + eps)^-1/2) U; (lambda, Y) = eigh(S M_f S^T); c_k = normalise(y_k S); d_k = normalise(c_k Q) with its
    component of largest magnitude positive (the sign goes to c_k too; without Q the rule is applied to c_k itself)."""
    M_f, M_b = np.asarray(M_f, dtype=np.float64), np.asarray(M_b, dtype=np.float64)
    eps = region_eps(M_f, M_b, reg)
    beta, Um = eigh_ref(M_b)
    S = ((np.maximum(beta, 0.0) + eps) ** -0.5)[:, None] * Um
    lam, Y = eigh_ref(S @ M_f @ S.T)
    c = Y @ S
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    if Q is None:
        return eps, lam, sign_rule(c), None
    d = c @ np.asarray(Q, dtype=np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    flipped = sign_rule(d)
    sign = np.where(np.sum(flipped * d, axis=1) < 0, -1.0, 1.0)[:, None]
    return eps, lam, c * sign, flipped


def rel_gaps(lam):
    """min_j |lam_k - lam_j| / lam_0 per k"""
    lam = np.asarray(lam, dtype=np.float64)
    d = np.abs(lam[:, None] - lam[None, :])
    np.fill_diagonal(d, np.inf)
    return d.min(axis=1) / lam[0]


def sin_angle(a, b):
    """sin of the angle between the rows of a and of b (unit or not), sign-free"""
    a = np.asarray(a, dtype=np.float64) / np.linalg.norm(a, axis=-1, keepdims=True)
    b = np.asarray(b, dtype=np.float64) / np.linalg.norm(b, axis=-1, keepdims=True)
    return np.linalg.norm(a - np.sum(a * b, axis=-1, keepdims=True) * b, axis=-1)


def rayleigh(u, M_f, M_b, eps):
    """R(u) = u M_f u^T / (u M_b u^T + eps |u|^2) per row of u, float64"""
    u = np.asarray(u, dtype=np.float64)
    M_f, M_b = np.asarray(M_f, dtype=np.float64), np.asarray(M_b, dtype=np.float64)
    return np.sum((u @ M_f) * u, axis=1) / (np.sum((u @ M_b) * u, axis=1) + eps * np.sum(u * u, axis=1))
