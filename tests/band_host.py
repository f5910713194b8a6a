"""Host references for the band factor's edges (csrc/band.hip): banded test systems with a known
tile width, the float64 LAPACK factor of S·PᵀAᵀA·P·S, one LSQR step on A·M with the triangular
solves done tile by tile (so that tiles can be left out to prove a test's sensitivity), and the
conditional σ of a window.  Host only: imported by tests/test_band_host.py and
tests/test_gpu_band_edges.py."""
import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

TB = 64
EPS = 2.0 ** -53                      # unit round-off of float64
LD = np.longdouble

# (n, reach) -> (T, w): the table of the cases; WIDE's ring, (w+1)·512 B, is above 64 KiB
CASES = {
    (40, 10): (1, 0),                 # single padded tile
    (64, 20): (1, 0),                 # n = 64 exactly, no padding
    (65, 3): (2, 1),                  # 63 padded rows
    (129, 128): (3, 2),               # w clipped to T − 1
    (768, 190): (12, 3),              # n = 12·64, NW = w
    (959, 450): (15, 8),              # w = NW cap exactly, no strided tile
    (897, 514): (15, 9),              # one strided tile, workgroup 0 only
    (1536, 1028): (24, 17),           # two strides plus a remainder, n = 24·64
    (1285, 1284): (21, 20),           # natural order, full band
    (8391, 8260): (132, 130),         # ring 67 072 B
}
WIDE = (8391, 8260)
SMALL = [c for c in CASES if c != WIDE]
NW_DEFAULT = 8
NW_VALUES = (1, 3, 8, 64)             # LSQ_BAND_NW values the GPU tests run (8: the default)
SEED = 1
DENSE_EIG_MAX = 2048                  # κ(Ñ) from eigvalsh up to here


def banded_system(n, reach, seed=SEED):
    """A = [diag(d); B] (scipy CSR, n + m_B rows), d ∈ [1, 2]; every row of B holds 3–5 entries
    (fewer only where its two ends are neighbours) of size 0.25 … 0.5 inside the columns
    [s, s + reach] of a start s.  The starts hold 0, n − 1 − reach and every 64k − 1 below it; the
    first row of each start has both end columns s and s + reach, so a row spans the widest tile
    distance the reach allows.  Then one row per band tile (I, J), its ends in tile I and tile J (tile
    row 0 of R̃ gets no fill, so only a direct entry keeps its tiles busy), then random rows over the
    starts in turn, at least 2n rows of B in all.  reach = 0: the diagonal alone."""
    rng = np.random.default_rng([seed, n, reach])
    d = rng.uniform(1.0, 2.0, n)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [d]
    smax = n - 1 - reach
    nb = 0
    if reach > 0 and smax >= 0:
        fixed = sorted({0, smax} | {s for s in range(TB - 1, smax + 1, TB)})
        free = np.setdiff1d(np.arange(smax + 1), fixed)
        extra = rng.choice(free, size=min(free.size, max(0, n // 8 - len(fixed))), replace=False)
        starts = np.r_[fixed, np.sort(extra)].astype(np.int64)
        T = (n + TB - 1) // TB
        w = min((reach + TB - 1) // TB, T - 1)
        pairs = [(I, J) for I in range(T) for J in range(I + 1, min(I + w, T - 1) + 1)]
        nb = max(2 * n, starts.size + len(pairs))

        def between(lo, hi, k):       # lo, hi and up to k − 2 columns between them
            mid = np.arange(lo + 1, hi)
            mid = rng.choice(mid, size=min(mid.size, k - 2), replace=False)
            return np.r_[lo, np.sort(mid), hi].astype(np.int64)

        for i in range(nb):
            k = int(min(rng.integers(3, 6), reach + 1))
            if i < starts.size:       # the start's first row: both ends
                s = int(starts[i])
                c = between(s, s + reach, k)
            elif i < starts.size + len(pairs):   # a direct entry in every band tile
                I, J = pairs[i - starts.size]
                c1 = int(rng.integers(I * TB, (I + 1) * TB))
                if c1 + reach < J * TB:
                    c1 = (I + 1) * TB - 1
                c2 = int(rng.integers(J * TB, min(n, (J + 1) * TB, c1 + reach + 1)))
                c = between(c1, c2, k)
            else:
                s = int(starts[i % starts.size])
                c = np.sort(rng.choice(np.arange(s, s + reach + 1), size=k, replace=False))
            rows.append(np.full(c.size, n + i))
            cols.append(c)
            vals.append(rng.uniform(0.25, 0.5, c.size) * rng.choice([-1.0, 1.0], c.size))
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n + nb, n))
    A.sort_indices()
    return A


def block_order(n, seed=SEED):
    """A band-preserving order: the reversal composed with a shuffle inside each 64-block of
    positions (a tile's columns stay one tile's columns, in reverse tile order)."""
    rng = np.random.default_rng([seed, n, 7])
    rev = np.arange(n - 1, -1, -1)
    out = rev.copy()
    for a in range(0, n, TB):
        out[a:a + TB] = rng.permutation(rev[a:a + TB])
    return out.astype(np.int32)


def edge_rhs(A, perm=None, seed=SEED):
    """(random b, b supported only on the rows that touch the first or the last tile)"""
    A = sp.csr_matrix(A)
    m, n = A.shape
    rng = np.random.default_rng([seed, n, 11])
    b = rng.standard_normal(m)
    pinv = np.empty(n, np.int64)
    pinv[np.arange(n) if perm is None else np.asarray(perm)] = np.arange(n)
    t = pinv[A.indices] >> 6
    edge = (t == 0) | (t == (n - 1) >> 6)
    hit = np.add.reduceat(edge, A.indptr[:-1]) > 0      # every row of A holds an entry
    return b, np.where(hit, rng.standard_normal(m), 0.0)


def tile_width(A, perm=None, keep=None):
    """(T, w) as k_band_width and band_factor form them: w = max over live rows of (last − first
    tile) of the row's columns in the order perm (new position -> column; shorter than n: a
    window, columns outside are skipped), clipped to T − 1."""
    A = sp.csr_matrix(A)
    n = A.shape[1]
    perm = np.arange(n) if perm is None else np.asarray(perm, dtype=np.int64)
    pinv = np.full(n, -1, np.int64)
    pinv[perm] = np.arange(perm.size)
    T = (perm.size + TB - 1) // TB
    w = 0
    for i in range(A.shape[0]):
        if keep is not None and not keep[i]:
            continue
        k = pinv[A.indices[A.indptr[i]:A.indptr[i + 1]]]
        k = k[k >= 0] >> 6
        if k.size:
            w = max(w, int(k.max() - k.min()))
    return T, min(w, T - 1)


class Factor:
    """S, R̃ (upper, Ñ = S·PᵀAᵀA·P·S = R̃ᵀR̃, float64 LAPACK), κ(Ñ), and x* of a right-hand side."""

    def __init__(self, A, perm=None, w_rows=None, keep=None):
        A = sp.csr_matrix(A)
        m, n = A.shape
        self.A, self.n, self.m = A, n, m
        self.perm = np.arange(n) if perm is None else np.asarray(perm, dtype=np.int64)
        self.rs = (np.ones(m) if w_rows is None else np.asarray(w_rows, float)) * \
                  (1.0 if keep is None else np.asarray(keep, float))
        self.Aw = (sp.diags(self.rs) @ A).tocsr()
        self.T, self.w = tile_width(A, self.perm, self.rs != 0)
        Ap = self.Aw[:, self.perm]
        N = (Ap.T @ Ap).toarray()
        self.S = 1.0 / np.sqrt(np.diag(N))
        Nt = N * self.S[:, None] * self.S[None, :]
        self.N = N
        if n <= DENSE_EIG_MAX:
            ev = sla.eigvalsh(Nt)
            self.R = sla.cholesky(Nt, lower=False, overwrite_a=True, check_finite=False)
            self.kappa = float(ev[-1] / ev[0])
        else:   # the wide case: eigvalsh of 8 391² takes most of a minute; both ends by Lanczos on
            # the sparse Ñ (Ritz values approach the ends from inside: κ short by ≤ 1e-5 relative)
            Ns = (sp.diags(self.S) @ (Ap.T @ Ap) @ sp.diags(self.S)).tocsr()
            self.R = sla.cholesky(Nt, lower=False, overwrite_a=True, check_finite=False)
            v0 = np.ones(n)
            hi = spla.eigsh(Ns, k=1, which='LA', tol=1e-5, v0=v0, return_eigenvectors=False)[0]
            lo = spla.eigsh(Ns, k=1, which='SA', tol=1e-5, v0=v0, return_eigenvectors=False)[0]
            self.kappa = float(hi / lo)

    def solve_normal(self, g):
        """(AwᵀAw)⁻¹ g through the factor (g and the result in the compact column order)"""
        t = self.S * np.asarray(g, float)[self.perm]
        t = sla.solve_triangular(self.R, t, trans='T', check_finite=False)
        t = sla.solve_triangular(self.R, t, check_finite=False)
        out = np.empty(self.n)
        out[self.perm] = self.S * t
        return out

    def xstar(self, b):
        return refined(self.Aw, self.rs * np.asarray(b, float), self.solve_normal)


def refined(Aw, bw, solve_normal):
    """The LS solution of Aw x ≈ bw from a normal-equations solve plus one refinement step whose
    residual and gradient are formed in np.longdouble; returned as longdouble."""
    C = sp.coo_matrix(Aw)
    x = solve_normal(Aw.T @ bw)
    v = C.data.astype(LD)
    r = bw.astype(LD)
    np.subtract.at(r, C.row, v * x.astype(LD)[C.col])
    g = np.zeros(Aw.shape[1], LD)
    np.add.at(g, C.col, v * r[C.row])
    return x.astype(LD) + solve_normal(g.astype(float)).astype(LD)


def xstar_lu(A, b, w_rows=None, keep=None):
    """x* without a dense factor (the wide case): sparse LU of the normal matrix plus the
    refinement step."""
    A = sp.csr_matrix(A)
    rs = (np.ones(A.shape[0]) if w_rows is None else np.asarray(w_rows, float)) * \
         (1.0 if keep is None else np.asarray(keep, float))
    Aw = (sp.diags(rs) @ A).tocsr()
    lu = spla.splu((Aw.T @ Aw).tocsc())
    return refined(Aw, rs * np.asarray(b, float), lu.solve)


def host_factor(A, perm=None, w_rows=None, keep=None):
    return Factor(A, perm, w_rows, keep)


def _tri(F, v, trans, drop):
    """R̃⁻¹ v (trans False: back substitution, tile row K takes the tiles (K, J), J = K+1 … K+w) or
    R̃⁻ᵀ v (forward, tile column K takes the tiles (I, K), I = K−w … K−1), tile by tile as
    k_band_bsub / k_band_fsub; drop(row tile, column tile) leaves a tile's product out."""
    n, T, w, R = F.n, F.T, F.w, F.R
    x = np.zeros(n)
    order = range(T) if trans else range(T - 1, -1, -1)
    for K in order:
        k0, k1 = K * TB, min(n, (K + 1) * TB)
        others = range(max(0, K - w), K) if trans else range(K + 1, min(K + w, T - 1) + 1)
        acc = np.zeros(k1 - k0)
        if drop is None:
            if len(others):
                o0, o1 = others[0] * TB, min(n, (others[-1] + 1) * TB)
                acc = R[o0:o1, k0:k1].T @ x[o0:o1] if trans else R[k0:k1, o0:o1] @ x[o0:o1]
        else:
            for J in others:
                if drop(J, K) if trans else drop(K, J):
                    continue
                j0, j1 = J * TB, min(n, (J + 1) * TB)
                acc = acc + (R[j0:j1, k0:k1].T @ x[j0:j1] if trans else R[k0:k1, j0:j1] @ x[j0:j1])
        x[k0:k1] = sla.solve_triangular(R[k0:k1, k0:k1], v[k0:k1] - acc, trans='T' if trans else 'N',
                                        check_finite=False)
    return x


def host_one_step(A, b, factor, x0=None, drop=None):
    """x after one LSQR step on A·M, M = P·S·R̃⁻¹, from x0 (None: 0), in float64 — what
    solve(b, precond=5, maxit=1, x0=x0) computes: y0 = R̃S⁻¹Pᵀx0, the step, x = M·y.  A and b
    unweighted; the factor's row scale is applied here."""
    F = factor
    Aw = F.Aw
    assert sp.csr_matrix(A).shape == Aw.shape
    bw = F.rs * np.asarray(b, float)

    def M(y):
        out = np.empty(F.n)
        out[F.perm] = F.S * _tri(F, y, False, drop)
        return out

    def Mt(t):
        return _tri(F, F.S * t[F.perm], True, drop)

    if x0 is None:
        y = np.zeros(F.n)
        u = bw.copy()
    else:
        x0 = np.asarray(x0, float)
        y = F.R @ (x0[F.perm] / F.S)
        u = bw - Aw @ x0
    beta1 = np.linalg.norm(u)
    u /= beta1
    v = Mt(Aw.T @ u)
    alpha1 = np.linalg.norm(v)
    if alpha1 == 0.0:
        return M(y)
    v /= alpha1
    u2 = Aw @ M(v) - alpha1 * u
    beta2 = np.linalg.norm(u2)
    rho = np.hypot(alpha1, beta2)
    phi = alpha1 / rho * beta1
    return M(y + (phi / rho) * v)


def rel_err(x, xs):
    """‖x − x*‖₂ / ‖x*‖₂, the difference formed in longdouble"""
    xs = np.asarray(xs, LD)
    return float(np.linalg.norm(np.asarray(x, LD) - xs) / np.linalg.norm(xs))


def bound(e_host, w, kappa):
    """The GPU tests' tolerance: 32 host errors, or the longest dot product of a tile row times unit
    round-off and the condition number (the device sums in 64-wide tiles in another order)."""
    return max(32.0 * e_host, 64.0 * (w + 1) * EPS * kappa)


def window_sigma(N, cols, inner=None):
    """sqrt(diag((N[cols][:, cols])⁻¹)) at the inner positions (None: all), 0 elsewhere; N dense or
    sparse, in the compact column order."""
    cols = np.asarray(cols, dtype=np.int64)
    Nw = N[cols][:, cols]
    Nw = Nw.toarray() if sp.issparse(Nw) else np.asarray(Nw)
    s = 1.0 / np.sqrt(np.diag(Nw))
    c = sla.cholesky(Nw * s[:, None] * s[None, :], lower=False, check_finite=False)
    Ri = sla.solve_triangular(c, np.eye(cols.size), check_finite=False)   # R̃⁻¹: Ñ⁻¹ = R̃⁻¹R̃⁻ᵀ
    sig = np.sqrt(np.sum(Ri * Ri, axis=1)) * s
    if inner is not None:
        sig = np.where(np.asarray(inner, bool), sig, 0.0)
    return sig


def op_sigma(N, op):
    """sqrt(diag(op N⁻¹ opᵀ)) for the rows of op (scipy sparse over the compact columns)"""
    N = N.toarray() if sp.issparse(N) else np.asarray(N)
    s = 1.0 / np.sqrt(np.diag(N))
    c = sla.cholesky(N * s[:, None] * s[None, :], lower=False, check_finite=False)
    Y = sla.solve_triangular(c, (sp.csr_matrix(op) @ sp.diags(s)).toarray().T, trans='T', check_finite=False)
    return np.sqrt(np.sum(Y * Y, axis=0))


@functools.lru_cache(maxsize=None)
def case(n, reach, order='natural', reweight=False):
    """(A, Factor, w_rows, keep) of a case, formed once per process.  order 'block': block_order.
    reweight: row weights in [0.5, 2] and 10 % of B's rows masked (the diagonal rows kept)."""
    A = banded_system(n, reach)
    perm = block_order(n) if order == 'block' else None
    w_rows = keep = None
    if reweight:
        rng = np.random.default_rng([SEED, n, reach, 13])
        w_rows = rng.uniform(0.5, 2.0, A.shape[0])
        keep = rng.random(A.shape[0]) > 0.1
        keep[:n] = True
    return A, Factor(A, perm, w_rows, keep), w_rows, keep
