"""The dense factor (dense.hip: N = AᵀA = RᵀR in 64 × 64 tiles, R⁻¹, E = sqrt(row sums of R⁻¹²)) and
the one LSQR step it preconditions (precond 2 in lsqr.hip) against tests/dense_host.py: a plain
right-looking Cholesky and a row-by-row back substitution in extended precision.

Tolerances, all from dense_host.Ref: rowdev(R⁻¹) = max_i ‖row_i − row_i^ld‖ / ‖row_i^ld‖ within
tau = max(1000·e, 1e-13) with e the float64 host run's own rowdev; E within tau_E, the same
construction on |E_i − E_ld,i| / E_ld,i; x_1 within tau_1 and r1norm, anorm, acond, xnorm within
their lsqr_host.Ref tolerances (floor 1e-12).  arnorm_1 is rounding noise (A·R⁻¹ has orthonormal
columns: LSQR is done after one step, see dense_host's docstring) and is bounded through
arnorm / (anorm·r1norm) ≤ max(1000 × the host float64 ratio, 1e-12).  tests/test_dense_host.py caps
e at 1e-14 and shows that each defect these tests are there for (a dropped kb term of k_trinv_row, an
un-updated k_syrk_tiles tile, padding that is not the identity, a masked row used, a stale factor,
R⁻¹ for R in the warm start) moves its metric by more than 100 tolerances.

Sizes: n = 1, 2, 63, 64, 65, 128, 129, 193, 257 (1 to 5 block rows, on and around the tile edge),
each plain and column-graded; the structured ksweep-9x11-2 through ensure_full_csr; n = 8200 in 164
independent blocks, whose rows 8192 … 8199 exist only in the grid-stride pass of k_gemv_upper and whose
538 MB R⁻¹ stays on the device (sigma_x() and the solves check it).

One handle takes one matrix: a second lsq_set_matrix_coo is refused ("matrix already set"), so the
dense buffers are never reused at another n with the same padded size.  test_refactoring_on_one_handle
asserts that refusal, refactors the one matrix under new weights and a new mask, and factors n = 100,
65 and 193 on fresh handles of the same process.

A solve with zero tolerances and maxit = 1 reports istop 7, or 5 when the noise arnorm_1 falls below
machine precision too (1 + arnorm/(anorm·r1norm) ≤ 1): k_givens restates scipy's order of the stopping
rules, in which that rule is tested after the iteration limit; scipy's own LSQR does the same on
these systems (tests/test_dense_host.py).

The figures go to the file named by DENSE_FACTOR_JSON, when set (profiles/dense_factor.json is one
such run, 43 entries).  Largest device / tolerance seen there: 0.0013 for R⁻¹ (63-graded: rowdev
8.9e-16 against e = 7.0e-16) and 0.0014 for E (n = 100: 1.0e-15 against e_E = 7.5e-16), 0.0060 for x_1
(ksweep-9x11-2 cold: 4.5e-15 against e_1 = 7.6e-16), 0.0023 for the eight rows of the second
k_gemv_upper pass, 0.0004 for a scalar (xnorm, wide cold) and 0.0007 for the arnorm ratio (7.4e-16
against the host's 3.4e-16, bound 1e-12): the device stays within a few e of the extended-precision
factor, and no defect was found in dense.hip or in the precond-2 branches of lsqr.hip."""
import atexit
import functools
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import conftest  # noqa: F401  (puts the repository root on sys.path)
import dense_host as D
import lsqr_host as L

pytestmark = pytest.mark.gpu
ZERO = dict(atol=0.0, btol=0.0, conlim=0.0, method=0)
STEP_SCALARS = ('r1norm', 'anorm', 'acond', 'xnorm')
GEMV_ROWS = 2048 * 4                      # k_gemv_upper: NPART workgroups of 4 rows in the first pass

RECORD = {}


def _dump_record():
    path = os.environ.get('DENSE_FACTOR_JSON')
    if path and RECORD:
        with open(path, 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


atexit.register(_dump_record)


def _open_coo(A, w, keep):
    import lssurf_amd as LS
    coo = sp.coo_matrix(A)
    s = LS.LSQSolver(0)
    try:
        s.set_matrix_coo(A.shape[0], A.shape[1], coo.row, coo.col, coo.data, row_weight=w)
        s.set_row_mask(keep)
    except BaseException:
        s.close()
        raise
    return s


def _open_structured(c):
    """The structured system of an lsqr_host case with its weights and mask
    (test_gpu_lsqr_iterates._open)."""
    from lssurf_amd.smooth_fit import FitSystem
    h = c.h
    fs = FitSystem(h.S['G_data'], h.S['Gc'], h.keep_cols, h.n_full, grids=h.S['grids'])
    try:
        assert fs.formation == 'stencil' and fs.solver.info()['stencil_op'] == 1
        fs.solver.set_row_weight(c.w)
        fs.solver.set_row_mask(c.mask)
    except BaseException:
        fs.close()
        raise
    return fs


def _check_factor(tag, r, Ri, E):
    """R⁻¹ (None: not downloaded) and E of a device factor against Ref r; the figures into RECORD."""
    rec = RECORD.setdefault(tag, {})
    bad = []
    if Ri is not None:
        assert Ri.shape == (r.n, r.n)
        assert np.count_nonzero(np.tril(Ri, -1)) == 0          # exact zeros: no leakage from a tile
        assert (np.diagonal(Ri) > 0).all()
        d = r.rowdev(Ri)
        rec['rinv'] = dict(device=d, e=r.e, tau=r.tau, ratio=d / r.tau)
        print(f'{tag}: rowdev {d:.2e}, e {r.e:.2e}, tau {r.tau:.2e}')
        if not d <= r.tau:
            bad.append(('rinv', d, r.tau))
    assert E.shape == (r.n,)
    dE = r.edev(E)
    rec['E'] = dict(device=dE, e=r.e_E, tau=r.tau_E, ratio=dE / r.tau_E)
    print(f'{tag}: E {dE:.2e}, e_E {r.e_E:.2e}, tau_E {r.tau_E:.2e}')
    if not dE <= r.tau_E:
        bad.append(('E', dE, r.tau_E))
    assert not bad, (tag, bad)


# ---- 1. R⁻¹ and E at every size --------------------------------------------------------------------
@pytest.mark.parametrize('name', D.NAMES)
def test_rinv_and_sigma_at_every_size(gpu_available, name):
    A, w, keep = D.inputs(name)
    with _open_coo(A, w, keep) as s:
        Ri, E = s.rinv(), s.sigma_x()
    _check_factor(name, D.ref(name), Ri, E)


# ---- 2. the structured formation -------------------------------------------------------------------
def test_structured_formation_reaches_the_same_factor(gpu_available):
    c = L.case(D.STRUCTURED)
    fs = _open_structured(c)
    try:
        E, Ri = fs.solver.sigma_x(), fs.solver.rinv()
    finally:
        fs.close()
    _check_factor(D.STRUCTURED, D.ref(D.STRUCTURED), Ri, E)


# ---- 3. refactoring ----------------------------------------------------------------------------------
def test_refactoring_on_one_handle(gpu_available):
    """New weights, then a new mask, on one handle: each factor against its own Ref (a stale factor
    is off by 1e11 tolerances: test_dense_host's stale_weights, masked_row_in).  The handle refuses a
    second matrix; n = 100, 65 (both padded to 128) and 193 then run on fresh handles one after the
    other, each against its own Ref."""
    from lssurf_amd._native import NativeError
    A, w, keep = D.system(100)
    w2, keep2 = D.weights_and_mask(A.shape[0], 3000)
    assert not np.array_equal(keep, keep2) and abs(w2 - w).max() > 0.5
    with _open_coo(A, w, keep) as s:
        _check_factor('refactor/100', D.Ref(A, w, keep), s.rinv(), s.sigma_x())
        s.set_row_weight(w2)
        _check_factor('refactor/100-weights', D.Ref(A, w2, keep), s.rinv(), s.sigma_x())
        s.set_row_mask(keep2)
        _check_factor('refactor/100-mask', D.Ref(A, w2, keep2), s.rinv(), s.sigma_x())
        B, wb, kb = D.system(65)
        coo = B.tocoo()
        with pytest.raises(NativeError, match='already set'):
            s.set_matrix_coo(B.shape[0], B.shape[1], coo.row, coo.col, coo.data, row_weight=wb)
        _check_factor('refactor/100-again', D.Ref(A, w2, keep2), s.rinv(), s.sigma_x())
    for n in (65, 193):
        B, wb, kb = D.system(n)
        with _open_coo(B, wb, kb) as s:
            _check_factor(f'refactor/{n}', D.ref(f'{n}-plain'), s.rinv(), s.sigma_x())


# ---- 4. one LSQR step with precond 2 -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _steps(name):
    """{(warm, batch): (x_1, stats)} and sigma_x() of a step case, one handle."""
    b = D.rhs(name)
    if name == D.STRUCTURED:
        fs = _open_structured(L.case(name))
        s, close = fs.solver, fs.close
    else:
        s = _open_coo(*D.inputs(name))
        close = s.close
    try:
        out = {}
        for warm in (False, True):
            for batch in (0, 2):
                x, st = s.solve(b, x0=D.warm_start(name) if warm else None, maxit=1, precond=2, batch=batch, **ZERO)
                assert st['method'] == 0 and st['iters'] == 1, st
                # maxit stops the solve (7) unless the noise arnorm_1 also falls below machine precision:
                # scipy's order of the stopping rules, which k_givens restates, then reports 5
                assert st['istop'] == 7 or (st['istop'] == 5 and 1.0 + D.arnorm_ratio(st, None) <= 1.0), st
                out[(warm, batch)] = (x, st)
        return out, s.sigma_x()
    finally:
        close()


@pytest.mark.parametrize('batch', [0, 2], ids=['batch16', 'batch2'])
@pytest.mark.parametrize('warm', [False, True], ids=['cold', 'warm'])
@pytest.mark.parametrize('name', D.STEP_CASES)
def test_one_step_with_the_dense_preconditioner(gpu_available, name, warm, batch):
    """maxit = 1 stops inside a batch (2: on its first of two iterations; 16: of sixteen), the owed
    x/w update paid by the rest of the batch or the flush; the warm start goes through y0 = R x0
    (k_gemv_upper mode 2 on S.dR)."""
    x, st = _steps(name)[0][(warm, batch)]
    ref = D.step(name, warm)
    tag = f'step/{name}/{"warm" if warm else "cold"}/batch{batch or 16}'
    rec = RECORD.setdefault(tag, {})
    rec['istop'] = st['istop']
    bad = []
    d = ref.dev(1, x)
    rec['x_1'] = dict(device=d, e=ref.e[1], tau=ref.tau[1], ratio=d / ref.tau[1])
    print(f'{tag}: x_1 {d:.2e}, e_1 {ref.e[1]:.2e}, tau_1 {ref.tau[1]:.2e}')
    if not d <= ref.tau[1]:
        bad.append(('x_1', d, ref.tau[1]))
    if x.size > GEMV_ROWS:                 # the rows only the grid-stride second pass of k_gemv_upper writes
        want = ref.ld['x'][1][GEMV_ROWS:]
        e2 = ref.dev(1, ref.f64['x'][1][GEMV_ROWS:], want)
        tau2 = max(1000 * e2, 1e-13)
        d2 = ref.dev(1, x[GEMV_ROWS:], want)
        rec['x_1_second_pass'] = dict(device=d2, e=e2, tau=tau2, ratio=d2 / tau2)
        print(f'{tag}: x_1[{GEMV_ROWS}:] {d2:.2e}, e {e2:.2e}, tau {tau2:.2e}')
        assert x.size - GEMV_ROWS == 8 and d2 <= tau2, ('rows of the second pass', d2, tau2)
    for f in STEP_SCALARS:
        ds = ref.sdev(f, 1, st[f])
        rec[f] = dict(device=ds, e=ref.es[f][1], tau=ref.taus[f][1], ratio=ds / ref.taus[f][1])
        print(f'{tag} {f}: device {ds:.2e}, e {ref.es[f][1]:.2e}, tau {ref.taus[f][1]:.2e}')
        if not ds <= ref.taus[f][1]:
            bad.append((f, ds, ref.taus[f][1]))
    host, dev = D.arnorm_ratio(ref.f64), D.arnorm_ratio(st, None)
    bound = max(1000 * host, 1e-12)
    rec['arnorm_ratio'] = dict(device=dev, host=host, bound=bound, ratio=dev / bound)
    print(f'{tag}: arnorm/(anorm r1norm) {dev:.2e}, host float64 {host:.2e}, bound {bound:.2e}')
    if not dev <= bound:
        bad.append(('arnorm ratio', dev, bound))
    assert not bad, (tag, bad)


def test_wide_system_sigma_against_its_block_references(gpu_available):
    r = D.ref('wide')
    assert r.n == 8200 > GEMV_ROWS and r.Ri_ld.shape == (D.WIDE_BLOCKS, D.WIDE_K, D.WIDE_K)
    _check_factor('wide', r, None, _steps('wide')[1])


# ---- 5. not positive definite is a refusal -----------------------------------------------------------
def _refused(s, b):
    from lssurf_amd._native import NativeError
    for call in (s.sigma_x, s.rinv, lambda: s.solve(b, precond=2)):
        with pytest.raises(NativeError, match='positive definite'):
            call()


def test_empty_columns_are_refused_and_the_handle_lives_on(gpu_available):
    """test_gpu_edge_cases.test_empty_columns_and_rows' 60 × 9 matrix (columns 2 and 7 empty): the
    dense factor refuses, then precond 1 solves on the same handle to that test's result."""
    from oracle import dense
    rng = np.random.default_rng(2)
    m, n = 60, 9
    A = sp.lil_matrix((m, n))
    for i in range(m):
        if i in (0, 5, 6):
            continue
        for j in rng.choice([0, 1, 3, 4, 5, 6, 8], size=3, replace=False):
            A[i, j] = rng.normal()
    A = A.tocsr()
    b = rng.normal(size=m)
    with _open_coo(A, None, np.ones(m, bool)) as s:
        _refused(s, b)
        x, st = s.solve(b, precond=1, atol=1e-13, btol=1e-13, conlim=1e14)
    live = np.array([0, 1, 3, 4, 5, 6, 8])
    xs = np.zeros(n)
    xs[live] = dense.ls_solve_dense(sp.csr_matrix(A[:, live]), b)
    assert st['istop'] in (1, 2), st
    assert x[2] == 0 and x[7] == 0
    assert np.linalg.norm(x - xs) / np.linalg.norm(xs) < 1e-9


def test_a_masked_out_column_is_refused_until_the_mask_lifts(gpu_available):
    """A full-rank matrix with every row that touches column 40 masked: refused; with every row kept
    the same handle factors and E meets tau_E."""
    A, w, _ = D.system(65)
    col = 40
    keep = np.ones(A.shape[0], bool)
    keep[A.tocsc()[:, col].indices] = False
    assert keep.sum() > A.shape[1] and np.linalg.matrix_rank(A.toarray()) == A.shape[1]
    b = D.rhs('65-plain')
    with _open_coo(A, w, keep) as s:
        _refused(s, b)
        s.set_row_mask(np.ones(A.shape[0], bool))
        E, Ri = s.sigma_x(), s.rinv()
    _check_factor('refused/65-unmasked', D.Ref(A, w, np.ones(A.shape[0], bool)), Ri, E)
