"""Host (numpy / scipy) reference of the dense factor (lssurf_amd/csrc/dense.hip) and of the one
LSQR step it preconditions (precond 2, lsqr.hip): N = (diag(w·keep)·A)ᵀ(diag(w·keep)·A) = RᵀR by a
plain right-looking Cholesky, R⁻¹ by back substitution row by row, E = sqrt(row sums of R⁻¹²), each
run in float64 and in extended precision from the float64 entries of A.  The device forms the same
quantities in 64 × 64 tiles (k_potrf_diag, k_trsm_panel, k_syrk_tiles, k_trinv_diag, k_trinv_row,
k_rowrss_dense), so it differs from these by the association of its sums alone.

The metric is per row: rowdev(X) = max_i ‖X[i,:] − R⁻¹_ld[i,:]‖ / ‖R⁻¹_ld[i,:]‖.  A row's norm is E_i,
the quantity handed to users, so a wrong tile cannot hide behind rows of larger entries as it can
in a Frobenius norm.  e is the float64 host run's own rowdev and the device must stay within
tau = max(1000·e, 1e-13); for E the same with |E_i − E_ld,i| / E_ld,i (e_E, tau_E).  Factor and floor
are those of tests/lsqr_host.py and tests/test_gpu_cgnr_iterates.py: they cover the device's other
association (blocked tiles, 4 × 4 register blocks, wave trees).

Only k = 1 of the preconditioned LSQR is pinned, and that is the whole story: A·R⁻¹ has orthonormal
columns, so v_1 = Qᵀu_1/α_1 already solves the problem, x_1 is the least-squares solution,
α_2 = ‖Qᵀu_2 − β_2 v_1‖ = 0 in exact arithmetic and the recurrence would terminate.  From k = 2 on
every vector is rounding noise divided by rounding noise; arnorm_1 = α_2·|τ| is noise already and gets
no relative tolerance, only a bound on arnorm / (anorm·r1norm).  Do not add k = 2, 3, 16, 17 by
analogy with the other iterate tests: there is nothing there to pin.  (tests/test_dense_host.py
asserts that x_1 is the normal-equations solution.)

Systems: n ∈ SIZES puts n on, just below and just above multiples of the tile of 64 with 1, 1, 1, 1,
2, 2, 3, 4, 5 block rows (k_trsm_panel and the ib < jb tiles of k_syrk_tiles need 3, the kb loop of
k_trinv_row needs 4 to sum three terms; 65, 129, 193, 257 leave one real column beside 63 identity
columns in the last tile), each plain (cond 2 … 7) and column-graded (cond ≈ 1e3); `wide`, n = 8200
in 164 independent 50-column blocks that straddle the tile edges, whose reference is 164 small
factors and whose rows from 8192 on exist only in the grid-stride second pass of k_gemv_upper
(2048 workgroups of 4 rows); and the structured lsqr_host case ksweep-9x11-2.
Test infrastructure only."""
import functools

import numpy as np
import scipy.sparse as sp

import lsqr_host as L

LD = np.longdouble
TB = 64                                   # dense.hip's tile edge
SIZES = (1, 2, 63, 64, 65, 128, 129, 193, 257)
BLOCK_ROWS = (1, 1, 1, 1, 2, 2, 3, 4, 5)
VARIANTS = ('plain', 'graded')
WIDE_BLOCKS, WIDE_K, WIDE_M = 164, 50, 203
STRUCTURED = 'ksweep-9x11-2'
NAMES = [f'{n}-{v}' for n in SIZES for v in VARIANTS]
ALL = NAMES + ['wide', STRUCTURED]


# ---- the factor routines ---------------------------------------------------------------------
def chol_upper(N, dtype, skip=None):
    """R (upper) with RᵀR = N, right-looking, in dtype.  skip = (kb, ib, jb) (the sensitivity tests
    alone): the columns of block kb leave tile (ib, jb), ib < jb, of the trailing matrix un-updated."""
    A = np.array(N, dtype)
    n = A.shape[0]
    R = np.zeros_like(A)
    for j in range(n):
        R[j, j:] = A[j, j:] / np.sqrt(A[j, j])
        U = np.outer(R[j, j + 1:], R[j, j + 1:])
        if skip is not None and j // TB == skip[0]:
            r0, c0 = skip[1] * TB - (j + 1), skip[2] * TB - (j + 1)
            assert r0 >= 0 and c0 > r0
            U[r0:r0 + TB, c0:c0 + TB] = 0
        A[j + 1:, j + 1:] -= U
    return R


def inv_upper(R, dtype):
    """R⁻¹ by back substitution, bottom row first, in dtype."""
    R = np.asarray(R, dtype)
    n = R.shape[0]
    Ri = np.zeros_like(R)
    for i in range(n - 1, -1, -1):
        row = -(R[i, i + 1:] @ Ri[i + 1:, :])
        row[i] += 1
        Ri[i, :] = row / R[i, i]
    return Ri


def normal(A_csc, s, cols, dtype):
    """(diag(s)·A[:, cols])ᵀ(diag(s)·A[:, cols]) in dtype from the float64 entries, over the rows that
    touch those columns."""
    sub = A_csc[:, cols]
    rows = np.unique(sub.indices)
    B = s[rows].astype(dtype)[:, None] * sub.tocsr()[rows].toarray().astype(dtype)
    return B.T @ B


class Ref:
    """The factor of one system: R_ld, Ri_ld, E_ld and their float64 twins R_64, Ri_64, E_64 (block:
    the columns fall into independent blocks of that many, every array then (blocks, k, k); else one
    block of n), the float64 run's own deviations e, e_E and the tolerances tau, tau_E."""

    def __init__(self, A, w, keep, block=None, w_prev=None):
        assert np.finfo(LD).eps < 1e-18
        self.A = sp.csr_matrix(A, dtype=np.float64)
        self.Ac = self.A.tocsc()
        self.m, self.n = self.A.shape
        self.w, self.keep, self.w_prev = np.asarray(w, np.float64), np.asarray(keep, bool), w_prev
        self.s = self.w * self.keep
        self.cols = np.arange(self.n).reshape(-1, block or self.n)
        self.N_ld, self.R_ld, self.Ri_ld = self.factor(LD)
        self.N_64, self.R_64, self.Ri_64 = self.factor(np.float64)
        assert self.Ri_ld.dtype == LD
        self.E_ld, self.E_64 = self.rowrss(self.Ri_ld), self.rowrss(self.Ri_64)
        self.e = max(self._rowdev(a, b) for a, b in zip(self.Ri_64, self.Ri_ld))
        self.e_E = self.edev(self.E_64)
        self.tau, self.tau_E = max(1000 * self.e, 1e-13), max(1000 * self.e_E, 1e-13)

    def factor(self, dtype, s=None, **kw):
        s = self.s if s is None else s
        N = [normal(self.Ac, s, c, dtype) for c in self.cols]
        R = [chol_upper(a, dtype, **kw) for a in N]
        return np.array(N), np.array(R), np.array([inv_upper(r, dtype) for r in R])

    def rowrss(self, Ri):
        out = np.zeros(self.n, Ri.dtype)
        out[self.cols] = np.sqrt((Ri * Ri).sum(axis=2))
        return out

    @staticmethod
    def _rowdev(X, want):
        X = np.asarray(X).astype(LD)
        if not np.isfinite(X).all():
            return np.inf
        return float((np.sqrt(((X - want) ** 2).sum(axis=1)) / np.sqrt((want ** 2).sum(axis=1))).max())

    def rowdev(self, X):
        """max_i ‖X[i,:] − Ri_ld[i,:]‖ / ‖Ri_ld[i,:]‖ (inf for a non-finite X)"""
        assert len(self.cols) == 1 and X.shape == (self.n, self.n)
        return self._rowdev(X, self.Ri_ld[0])

    def edev(self, E):
        """max_i |E_i − E_ld,i| / E_ld,i (inf for a non-finite E)"""
        E = np.asarray(E).astype(LD)
        return float((abs(E - self.E_ld) / self.E_ld).max()) if np.isfinite(E).all() else np.inf

    # ---- the one LSQR step ---------------------------------------------------------------------
    @property
    def factors(self):
        """Ri_ld in lsqr_host.lsqr's format (rounded to float64 by its float64 run)"""
        return [(self.cols, self.Ri_ld)]

    def weighted(self, b):
        """(A_w, b_w): the kept rows of diag(w)·A and of w∘b"""
        rows = np.flatnonzero(self.keep)
        return sp.csr_matrix(sp.diags(self.w) @ self.A)[rows], (self.w * b)[rows]

    def step(self, b, x0=None):
        """lsqr_host.Ref of one step from x0 on this system with M = Ri_ld."""
        A_w, b_w = self.weighted(b)
        return L.Ref(A_w, b_w, self.factors, 1, x0=x0)

    def solution(self, b, dtype=LD):
        """R⁻¹R⁻ᵀ A_wᵀ b_w from R_ld, in dtype"""
        A_w, b_w = self.weighted(b)
        g = np.zeros(self.n, LD)
        g[:] = A_w.astype(LD).T @ b_w.astype(LD)
        return L.apply_m(self.factors, L.apply_mt(self.factors, g)).astype(dtype)


def arnorm_ratio(out, k=1):
    """arnorm_k / (anorm_k · r1norm_k) of an lsqr_host.lsqr result (or a device stats dict, k None)"""
    if k is None:
        return float(out['arnorm'] / (out['anorm'] * out['r1norm']))
    return float(out['arnorm'][k] / (out['anorm'][k] * out['r1norm'][k]))


# ---- defects (tests/test_dense_host.py: each moves its metric by more than 100 tolerances) -----
DEFECTS = ('drop_kb', 'skip_syrk_tile', 'pad_not_identity', 'masked_row_in', 'stale_weights', 'r_for_ri_warm')


def defective(ref, name, step=None):
    """The float64 R⁻¹ of ref (for r_for_ri_warm: x_1 of `step`, an lsqr_host.Ref with a warm start)
    with one defect applied:
    drop_kb           tile (0, last) of R⁻¹ = −R⁻¹_00 Σ_kb R[0, kb] R⁻¹[kb, last] without its kb = 1 term
    skip_syrk_tile    the Cholesky's first block step leaves trailing tile (1, 2) un-updated
    pad_not_identity  the last tile factored with zeros, not ones, on the padding diagonal: the plain
                      arithmetic divides 0 by 0 there and R⁻¹ comes out non-finite (k_potrf_diag itself
                      takes such a pivot as 1 and raises its error flag)
    masked_row_in     the masked row of largest weighted norm used after all
    stale_weights     the factor of the weights before (ref.w_prev)
    r_for_ri_warm     warm start y0 = R⁻¹x0 where R x0 belongs: x_1 = R⁻¹(y0 + t_1 w_1)"""
    assert name in DEFECTS
    if name == 'r_for_ri_warm':
        Ri, x0 = ref.Ri_64[0], step.x0
        return step.f64['x'][1] - x0 + Ri @ (Ri @ x0)
    assert len(ref.cols) == 1
    n, nb = ref.n, -(-ref.n // TB)
    if name == 'drop_kb':
        assert nb >= 3
        R, Ri = ref.R_64[0], ref.Ri_64[0].copy()
        t = [slice(k * TB, min((k + 1) * TB, n)) for k in range(nb)]
        acc = sum(R[t[0], t[kb]] @ Ri[t[kb], t[-1]] for kb in range(2, nb))
        Ri[t[0], t[-1]] = -Ri[t[0], t[0]] @ acc
        return Ri
    if name == 'skip_syrk_tile':
        assert nb >= 3
        with np.errstate(invalid='ignore'):       # a pivot may come out negative: R⁻¹ is then non-finite
            return ref.factor(np.float64, skip=(0, 1, 2))[2][0]
    if name == 'pad_not_identity':
        assert n % TB
        Np = np.zeros((nb * TB, nb * TB))
        Np[:n, :n] = ref.N_64[0]
        with np.errstate(all='ignore'):
            return inv_upper(chol_upper(Np, np.float64), np.float64)[:n, :n]
    if name == 'masked_row_in':
        out = np.flatnonzero(~ref.keep)
        norms = ref.w[out] * np.sqrt(np.asarray(ref.A[out].multiply(ref.A[out]).sum(axis=1)).ravel())
        s = ref.s.copy()
        s[out[np.argmax(norms)]] = ref.w[out[np.argmax(norms)]]
        return ref.factor(np.float64, s=s)[2][0]
    assert ref.w_prev is not None
    return ref.factor(np.float64, s=ref.w_prev * ref.keep)[2][0]


# ---- the inputs the CPU and GPU tests share ----------------------------------------------------
def weights_and_mask(m, seed):
    """row weights U(0.5, 2) and a mask that drops about 10 % of the rows"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2, m), rng.random(m) > 0.1


@functools.lru_cache(maxsize=None)
def system(n, variant='plain'):
    """(A (4n + 3) × n in CSR, w, keep), seeded by n: sp.random of about 6 entries per row plus the
    identity; `graded` scales column j by 10^(−3j/(n−1))."""
    m = 4 * n + 3
    rng = np.random.default_rng(1000 + n)
    A = sp.random(m, n, density=min(1.0, 6.0 / n), random_state=rng, format='csr') + sp.eye(m, n, format='csr')
    if variant == 'graded':
        A = A @ sp.diags(np.logspace(0, -3, n))
    w, keep = weights_and_mask(m, 2000 + n)
    return sp.csr_matrix(A), w, keep


@functools.lru_cache(maxsize=None)
def wide_system():
    """n = 8200: 164 independent blocks of 203 × 50 on the diagonal."""
    rng = np.random.default_rng(8200)
    A = sp.block_diag([sp.random(WIDE_M, WIDE_K, density=6.0 / WIDE_K, random_state=rng) + sp.eye(WIDE_M, WIDE_K)
                       for _ in range(WIDE_BLOCKS)], format='csr')
    w, keep = weights_and_mask(A.shape[0], 8201)
    return A, w, keep


def inputs(name):
    """(A unweighted, w, keep) of a system of ALL; the structured case's are its Host's G, the
    case's weights and its mask."""
    if name == 'wide':
        return wide_system()
    if name == STRUCTURED:
        c = L.case(name)
        return c.h.G, c.w, c.mask
    n, variant = name.split('-')
    return system(int(n), variant)


@functools.lru_cache(maxsize=None)
def ref(name):
    return Ref(*inputs(name), block=WIDE_K if name == 'wide' else None)


def rhs(name):
    """b with a residual: standard normal over every row (m > 4n, so b is far from range(A))."""
    return np.random.default_rng(31).standard_normal(inputs(name)[0].shape[0])


def warm_start(name):
    """the solution with every entry perturbed by 10 % of itself times a standard normal"""
    x = ref(name).solution(rhs(name), np.float64)
    return x * (1 + 0.1 * np.random.default_rng(37).standard_normal(x.size))


@functools.lru_cache(maxsize=None)
def step(name, warm):
    """lsqr_host.Ref of the one step on a system, cold or from warm_start."""
    return ref(name).step(rhs(name), warm_start(name) if warm else None)


STEP_CASES = ['129-plain', '257-plain', STRUCTURED, 'wide']
