"""Host (numpy / scipy) LSQR for the iterate tests of lsq method 0 (lssurf_amd/csrc/lsqr.hip,
lsqr_mf.inc, lsqr_block.inc): Paige & Saunders' LSQR on A·M written from the definitions, M applied
from the right per column block — 1 (precond 0), 1/‖A_j‖ (precond 1) or x = R̃ y with R̃ the upper
R_b⁻¹ of (AᵀA)_bb = R_bᵀR_b rounded to bf16 as the device keeps it (precond 3) — run in float64 or
in extended precision, with the recurrence scalars of scipy.sparse.linalg.lsqr that k_beta and
k_givens restate.  With the factors rounded alike the device's iterates differ from these by
summation order alone.  Also the inputs (systems, masks, weights, warm starts) that
tests/test_lsqr_host.py and tests/test_gpu_lsqr_iterates.py share, and the LDS sum that decides
which side of MF_LDS_MAX a grid's A·v falls on.

LDS sums (doubles; assemble.hip: Σ over used y offsets of MF_ALIGN + span; staged when ≤ 4096), per
grid of each case (tests/test_lsqr_host.py asserts them):
    every case's z0 grid                    1542            staged
    t64, t64-mask, t64-rows, t64-x0, ta64   dz 1575         staged
    sf3d 1557, nb_xt 1566, ksweep-9x11-2 1545, ksweep-9x11-5 1554, ksweep-7x70-13 1578    staged
    hbm (a 5 × 9 lattice of 860 epochs)     dz 4119         gathered from HBM
Test infrastructure only."""
import functools

import numpy as np
import scipy.sparse as sp

import cgnr_host as H

SCALARS = ('r1norm', 'anorm', 'acond', 'arnorm', 'xnorm')


# ---- the reference ---------------------------------------------------------------------------
def identity_factors(n):
    """1×1 factors 1 (precond 0)."""
    return [(np.arange(n)[:, None], np.ones((n, 1, 1)))]


def apply_m(factors, y):
    """x = M y = R̃ y block by block, in y's precision."""
    x = np.zeros_like(y)
    for C, Ri in factors:
        x[C] = (Ri.astype(y.dtype) * y[C][:, None, :]).sum(axis=2)
    return x


def apply_mt(factors, s):
    """Mᵀ s = R̃ᵀ s block by block, in s's precision."""
    y = np.zeros_like(s)
    for C, Ri in factors:
        y[C] = (Ri.astype(s.dtype) * s[C][:, :, None]).sum(axis=1)
    return y


def m_explicit(factors, n):
    """M as a sparse matrix (float64)."""
    rows, cols, vals = [], [], []
    for C, Ri in factors:
        k = C.shape[1]
        rows.append(np.repeat(C, k, axis=1).ravel())
        cols.append(np.tile(C, (1, k)).ravel())
        vals.append(np.asarray(Ri, np.float64).ravel())
    M = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    M.eliminate_zeros()
    return M


def _sym_ortho(a, b):
    """scipy's _sym_ortho: the stable Givens rotation (c, s, r)."""
    if b == 0:
        return np.sign(a), 0 * a, abs(a)
    if a == 0:
        return 0 * a, np.sign(b), abs(b)
    if abs(b) > abs(a):
        tau = a / b
        s = np.sign(b) / np.sqrt(1 + tau * tau)
        return s * tau, s, b / s
    tau = b / a
    c = np.sign(a) / np.sqrt(1 + tau * tau)
    return c, c * tau, a / c


DEFECTS = ('mt_swap', 'stale_v', 'cs_twice')


def lsqr(A, b, factors, kmax, x0=None, dtype=np.float64, defect=None, stale_cols=None):
    """kmax steps of LSQR on min ‖A M y − (b − A x0)‖, x_k = x0 + M y_k.  Returns a dict: x
    (kmax + 1, n) with x[k] the iterate after k steps, and per scalar of SCALARS an array (kmax + 1)
    with entry k the value scipy.sparse.linalg.lsqr(A·M, b − A x0, iter_lim=k) returns (entry 0:
    the set-up's; xnorm is ‖y_k‖, the correction in the preconditioned coordinates).
    defect (the sensitivity tests alone): 'mt_swap' applies R̃ where R̃ᵀ belongs in the Aᵀ leg,
    'stale_v' forms w_{k+1} from the ṽ of the step before (stale_cols, a column mask: on those columns
    alone — tests/dist_host.py: a rank's ghost copies left unexchanged), 'cs_twice' applies M twice in
    the A leg."""
    assert defect is None or defect in DEFECTS
    A = sp.csr_matrix(A).astype(dtype)
    AT = A.T.tocsr()
    b = np.asarray(b).astype(dtype)
    n = A.shape[1]
    one = dtype(1)

    def fwd(v):
        z = apply_m(factors, v)
        return A @ (apply_m(factors, z) if defect == 'cs_twice' else z)

    def adj(u):
        t = AT @ u
        return apply_m(factors, t) if defect == 'mt_swap' else apply_mt(factors, t)

    def norm(a):
        return np.sqrt(a @ a)

    x0 = np.zeros(n, dtype) if x0 is None else np.asarray(x0).astype(dtype)
    y = np.zeros(n, dtype)
    u = b - A @ x0
    beta = norm(u)
    u = u / beta
    v = adj(u)
    alfa = norm(v)
    v = v / alfa
    w = v.copy()
    v_prev = v
    rhobar, phibar = alfa, beta
    anorm = ddnorm = xxnorm = z = sn2 = res2 = 0 * one
    cs2 = -one
    out = {f: [0 * one] for f in SCALARS}
    out['r1norm'][0], out['arnorm'][0] = beta, alfa * beta
    xs = [x0.copy()]
    for _ in range(kmax):
        u = fwd(v) - alfa * u
        beta = norm(u)
        u = u / beta
        anorm = np.sqrt(anorm * anorm + alfa * alfa + beta * beta)
        v_prev, v = v, adj(u) - beta * v
        alfa = norm(v)
        v = v / alfa
        cs, sn, rho = _sym_ortho(rhobar, beta)
        theta = sn * alfa
        rhobar = -cs * alfa
        phi = cs * phibar
        phibar = sn * phibar
        tau = sn * phi
        t1, t2 = phi / rho, -theta / rho
        ddnorm = ddnorm + (w @ w) / (rho * rho)
        y = y + t1 * w
        w = ((v_prev if stale_cols is None else np.where(stale_cols, v_prev, v)) if defect == 'stale_v' else v) + t2 * w
        delta = sn2 * rho
        gambar = -cs2 * rho
        rhs = phi - delta * z
        zbar = rhs / gambar
        xnorm = np.sqrt(xxnorm + zbar * zbar)
        gamma = np.sqrt(gambar * gambar + theta * theta)
        cs2, sn2 = gambar / gamma, theta / gamma
        z = rhs / gamma
        xxnorm = xxnorm + z * z
        rnorm = np.sqrt(phibar * phibar + res2)
        for f, val in (('r1norm', rnorm), ('anorm', anorm), ('acond', anorm * np.sqrt(ddnorm)),
                       ('arnorm', alfa * abs(tau)), ('xnorm', xnorm)):
            out[f].append(val)
        xs.append(x0 + apply_m(factors, y))
    res = {f: np.array(out[f], dtype) for f in SCALARS}
    res['x'] = np.array(xs)
    return res


class Ref:
    """The reference iterates of one system in float64 and extended precision; of x_k the spread
    e_k = ‖x_k^f64 − x_k^ld‖ / ‖x_k^ld‖ and the tolerance τ_k = max(1000·e_k, 1e-13); of every scalar
    the same construction with floor 1e-12 (es[f][k], taus[f][k])."""

    def __init__(self, A, b, factors, kmax, x0=None):
        self.A, self.b, self.factors, self.x0, self.kmax = A, b, factors, x0, kmax
        self.f64 = lsqr(A, b, factors, kmax, x0=x0)
        self.ld = lsqr(A, b, factors, kmax, x0=x0, dtype=np.longdouble)
        assert self.ld['x'].dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18
        ks = range(1, kmax + 1)
        self.e = {k: self.dev(k, self.f64['x'][k]) for k in ks}
        self.tau = {k: max(1000 * e, 1e-13) for k, e in self.e.items()}
        self.es = {f: {k: self.sdev(f, k, self.f64[f][k]) for k in ks} for f in SCALARS}
        self.taus = {f: {k: max(1000 * e, 1e-12) for k, e in self.es[f].items()} for f in SCALARS}

    def dev(self, k, x, ref=None):
        """‖x − x_k^ld‖ / ‖x_k^ld‖"""
        return H.rel(np.asarray(x).astype(np.longdouble), self.ld['x'][k] if ref is None else ref)

    def sdev(self, f, k, value):
        """|value − f_k^ld| / |f_k^ld|"""
        want = self.ld[f][k]
        return float(abs(np.longdouble(value) - want) / abs(want))


# ---- which side of MF_LDS_MAX ----------------------------------------------------------------------
MF_ALIGN, MF_LDS_MAX = 512, 4096     # system.hpp (tests/test_lsqr_host.py reads them there)


def lds_sums(G_data, Gc):
    """{grid name: doubles of LDS its staged zv bands would take}: per used template y offset one band
    of MF_ALIGN + (largest − smallest in-row offset ox·nt + ot), summed (describe_stencil_operator in
    assemble.hip).  A grid whose sum exceeds MF_LDS_MAX gathers from HBM in k_mf_fwd."""
    from lssurf_amd.assemble import describe
    grids, _, _, stencils, _, fields = describe(G_data, Gc, with_fields=True)
    field_off = {k: off for k, off, _, _, _ in fields}
    names = {}
    for op in (G_data, Gc):
        for p in op.parts:
            names.setdefault(int(p['grid'].col_0), p['grid'].name)
    span = [{} for _ in grids]
    for i, s in enumerate(stencils):
        g = grids[s.grid]
        nt = int(g.shape[2]) if g.ndim == 3 else 1
        offs = field_off[i] if i in field_off else [[s.off[t][d] for d in range(3)] for t in range(s.ntpl)]
        for o in offs:
            oy, e = int(o[0]), int(o[1]) * nt + (int(o[2]) if g.ndim == 3 else 0)
            lo, hi = span[s.grid].get(oy, (e, e))
            span[s.grid][oy] = (min(lo, e), max(hi, e))
    return {names.get(int(g.col0), f'grid{k}'): sum(MF_ALIGN + hi - lo for lo, hi in span[k].values())
            for k, g in enumerate(grids) if span[k]}


# ---- the inputs the CPU and GPU tests share ----------------------------------------------------
K = (1, 2, 3, 15, 16, 17, 32, 33)   # batch 16: stops on the first, a middle and the last (flush) iteration
K4 = (1, 2, 3, 17)                  # of a batch, both ṽ parities, the first batch and the third
KB = (1, 2, 3, 4, 5)                # the batching tests: batches of 2 and 4
ROWS_SEED = 17
HBM_SHAPE, HBM_NPTS, HBM_NT = (5, 9), 300, 860
SMALL = ['ksweep-9x11-2', 'ksweep-9x11-5', 'ksweep-7x70-13', 'sf3d', 'lin2d', 'nb_xt']
CASES = ['t64', 't64-mask', 't64-rows', 't64-x0', 'ta64', 'hbm'] + SMALL
BLOCK_CASES = [c for c in CASES if c != 'hbm']      # hbm's 859-column nodes take no block factor: precond 0, 1


class _Lin2d(H.Host):
    """tests/golden sys_lin2d rebuilt with lin_op as test_gpu_cgnr._lin2d_structured builds it."""

    def __init__(self):
        from conftest import golden
        from lssurf_amd.fd_grid import fd_grid
        from lssurf_amd.lin_op import lin_op
        g = golden('sys_lin2d.npz')
        grid = fd_grid([[0., 2300.], [0., 2300.]], [100., 100.], name='z0')
        G = lin_op(grid, name='interp_z').interp_mtx([g['in_y'], g['in_x']])
        root = np.sqrt(np.prod(grid.delta))
        g2 = lin_op(grid, name='grad2_z0').grad2(DOF='z0')
        g1 = lin_op(grid, name='grad_z0').grad(DOF='z0')
        Gc = lin_op(None, name='constraints').vstack([g2, g1])
        self.S = {'G_data': G, 'Gc': Gc, 'grids': {'z0': grid}}
        self.keep_cols = np.arange(G.col_N)
        self.n_full, self.n_data = int(G.col_N), int(G.N_eq)
        self.w = 1. / np.concatenate([g['in_sigma'], 0.03 / root * np.ones(g2.N_eq), 75. / root * np.ones(g1.N_eq)])
        self.rhs = np.concatenate([g['in_z'], np.zeros(Gc.N_eq)])
        self.blocks = (None, None)           # no dz grid: precond 3 takes singletons


@functools.lru_cache(maxsize=None)
def system(name):
    """The Host of a case's system."""
    if name.startswith('t64'):
        return H.synthetic_host('t64')
    if name == 'ta64':
        from lssurf_amd import synthetic
        S, kw = synthetic.aniso_system('ta64')
        return H.Host(S, kw['reference_epoch'])
    if name == 'hbm':
        return H.ksweep_host(HBM_SHAPE, HBM_NPTS, HBM_NT)
    if name.startswith('ksweep'):
        shape, nt = name.split('-')[1:3]
        shape = tuple(int(v) for v in shape.split('x'))
        return H.ksweep_host(shape, dict(H.KSWEEP)[shape], int(nt))
    if name == 'lin2d':
        return _Lin2d()
    return H.golden_host(name)


def rows_weights(h):
    """The `t64-rows` case: mask_and_weights with the constraint rows' weights × U(0.5, 2) as well, so
    that no stencil part has one row scale (MfPart::wconst = 0 for every part)."""
    w, mask = H.mask_and_weights(h)
    w = w.copy()
    w[h.n_data:] *= np.random.default_rng(ROWS_SEED).uniform(0.5, 2, w.size - h.n_data)
    return w, mask


class Case:
    """One case of the table: the Host h, row weights w, row mask over every row, warm start x0 (or
    None), the host-formed A (weighted, selected rows) and b, and its references per preconditioner."""

    def __init__(self, name):
        self.name, self.h = name, system(name)
        h = self.h
        self.w, self.mask = h.w, np.ones(h.w.size, bool)
        if name == 't64-mask':
            self.w, self.mask = H.mask_and_weights(h)
        if name == 't64-rows':
            self.w, self.mask = rows_weights(h)
        self.x0 = H.warm_start(h) if name == 't64-x0' else None
        self.A = h.A(self.w, self.mask)
        self.b = (self.w * h.rhs)[self.mask]
        self._refs = {}

    @property
    def blocks(self):
        return H.block_list(*self.h.blocks, self.h.keep_cols.size)

    def factors(self, precond, round=True):
        if precond == 0:
            return identity_factors(self.A.shape[1])
        if precond == 1:
            return H.jacobi_factors(self.A)
        assert precond == 3
        return H.block_factors(self.A, self.blocks, round)

    def ref(self, precond, kmax):
        """Ref of this case with this preconditioner to kmax steps at least (computed once)."""
        have = self._refs.get(precond)
        if have is None or have.kmax < kmax:
            have = self._refs[precond] = Ref(self.A, self.b, self.factors(precond), kmax, x0=self.x0)
        return have

    def lds(self):
        return lds_sums(self.h.S['G_data'], self.h.S['Gc'])


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
