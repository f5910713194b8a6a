"""Extra sparse rows behind the stencil rows (lsq_set_extra_rows; csrc/xrows.inc) and smooth_fit's
prior_args / prior_edge_args on top of them.

Operator: lsq_normal_apply with extra rows must equal AᵀA p + XᵀW²X p, A = get_csr() of a second
handle WITHOUT extra rows and X the host scipy CSR of the rows (so the reference never passes through
the new formation), to the normal operator's own tolerance, 1e-12 of max|q| (test_gpu_cgnr.py:69).
Solves: the reference's recorded tile-edge system (tests/golden/sys_prior_edge.npz,
gen_golden_prior.py) within the project's REL 1e-6 / ABS 1e-4; smooth_fit against the reference's
outputs at the tolerances of test_gpu_bias.py's smooth_fit cases, with zero edit flips."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import lssurf_amd as LS
from conftest import golden, golden_points
from lssurf_amd._native import NativeError
from lssurf_amd.constraint_functions import node_column_blocks_affine, reference_epoch_keep_cols
from lssurf_amd.smooth_fit import FitSystem
from lssurf_amd.solver import LSQSolver
from priors_common import prior_kwargs
from test_gpu_bias import _host_reduced, _layouts
from test_gpu_cgnr import _profiler_runs_real_iterations, _times_are_positive

pytestmark = pytest.mark.gpu
REL, ABS = 1e-6, 1e-4
TOL = dict(atol=1e-12, btol=1e-12, conlim=1e12)
BLOCK = 256


@functools.lru_cache(maxsize=None)
def _base():
    """Host objects of synthetic t64 (64 × 64 × 12 grid, 8 192 points), a random data-row mask, and
    the weighted, row-selected A of a handle that never saw an extra row.  Shared, never changed."""
    from lssurf_amd import synthetic
    D, kw = synthetic.points('t64')
    S = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw)
    keep_cols = reference_epoch_keep_cols(S['G_data'].col_N, S['grids']['dz'], kw['reference_epoch'])
    w = 1. / np.concatenate((S['Ed'], S['Ec']))
    rhs = np.zeros(w.size)
    rhs[:S['data'].size] = S['data'].z
    keep = np.random.default_rng(21).random(S['data'].size) > 0.2
    fs = FitSystem(S['G_data'], S['Gc'], keep_cols, S['Gc'].col_N, grids=S['grids'])
    try:
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(np.concatenate([keep, np.ones(fs.n_con, bool)]))
        A = fs.solver.get_csr()
    finally:
        fs.close()
    for a in (w, rhs, keep, keep_cols):
        a.flags.writeable = False
    return S, kw, keep_cols, w, rhs, keep, A


def _system(extra_csr=None):
    S, kw, keep_cols, w, rhs, keep, A = _base()
    return FitSystem(S['G_data'], S['Gc'], keep_cols, S['Gc'].col_N, grids=S['grids'], extra_csr=extra_csr)


def _cols():
    S, kw, keep_cols = _base()[:3]
    gz, gd = S['grids']['z0'], S['grids']['dz']
    z0 = np.arange(gz.col_0, gz.col_0 + int(np.prod(gz.shape)))
    dz = np.arange(gd.col_0, gd.col_0 + int(np.prod(gd.shape)))
    removed = np.setdiff1d(np.arange(S['Gc'].col_N), keep_cols)
    return z0, dz, removed


def _csr(rows):
    """(indptr, cols, vals) of a list of (cols, vals) rows"""
    ip = np.r_[0, np.cumsum([len(c) for c, _ in rows])].astype(np.int64)
    return ip, np.concatenate([np.asarray(c, np.int64) for c, _ in rows] + [np.zeros(0, np.int64)]), \
        np.concatenate([np.asarray(v, float) for _, v in rows] + [np.zeros(0)])


def _random_rows(rng, n):
    """rows of 1 … 16 entries over the z0 and dz columns, removed columns among them"""
    z0, dz, removed = _cols()
    every = np.r_[z0, dz]
    rows = []
    for _ in range(n):
        k = int(rng.integers(1, 17))
        rows.append((rng.choice(every, k, replace=False), rng.standard_normal(k)))
    return rows


def _special_rows(rng):
    """every special case of the formation and of the lane / wave edges in one set of rows"""
    z0, dz, removed = _cols()
    kept_dz = np.setdiff1d(dz, removed)
    hot, warm = int(kept_dz[5000]), int(kept_dz[100])
    rows = _random_rows(rng, 40)
    rows.append((removed[:8], rng.standard_normal(8)))                       # every entry in a removed column
    rows.append(([hot, int(z0[7]), hot], [1.5, 2.0, -1.5]))                   # a duplicate pair that sums to zero
    rows.append(([warm, int(z0[9]), warm, warm], [1.0, 0.5, 2.0, 0.25]))      # duplicates that sum to non-zero
    rows.append(([int(z0[11]), int(kept_dz[17])], [0.0, 3.0]))                # an explicit zero
    rows.append(([int(kept_dz[3])], [0.0]))                                   # … that leaves the row empty
    rows.append((np.r_[z0[100:104], kept_dz[200:204]], rng.standard_normal(8)))   # z0 and dz columns
    rows.append((kept_dz[1000:1032], rng.standard_normal(32)))               # the widest row allowed
    for _ in range(300):                                                      # one column in 300 rows
        rows.append(([hot, int(rng.choice(kept_dz))], rng.standard_normal(2)))
    for _ in range(64 * 2 + 1):                                               # one in 64·k + 1 rows
        rows.append(([int(rng.choice(z0)), warm], rng.standard_normal(2)))
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]


def _host_X(csr, keep_cols, n_full):
    ip, cols, vals = csr
    X = sp.csr_matrix((vals, cols, ip), shape=(ip.size - 1, n_full))   # scipy sums the duplicates
    return X[:, keep_cols].tocsr()


def _check_operator(csr, rng, name, mask_x):
    S, kw, keep_cols, w, rhs, keep, A = _base()
    m_x = csr[0].size - 1
    wx = rng.uniform(0.5, 20., m_x)
    kx = rng.random(m_x) > 0.25 if mask_x else np.ones(m_x, bool)
    Xk = _host_X(csr, keep_cols, S['Gc'].col_N)
    fs = _system(csr)
    try:
        assert fs.formation == 'stencil' and fs.n_extra == m_x
        fs.solver.set_row_weight(np.r_[w, wx])
        fs.solver.set_row_mask(np.concatenate([keep, np.ones(fs.n_con - m_x, bool), kx]))
        ok, why = fs.solver.cg_available(1)
        assert ok, why
        m, n, nnz = fs.solver.shape()
        Xw = sp.diags(wx[kx]) @ Xk[kx]
        Xw.eliminate_zeros()
        assert (m, n) == (A.shape[0] + int(kx.sum()), A.shape[1]) and nnz == A.nnz + Xw.nnz, name
        for _ in range(2):
            pc = rng.standard_normal(A.shape[1])
            pf = np.zeros(fs.n_full)
            pf[keep_cols] = pc
            q = fs.solver.normal_apply(pf)[keep_cols]
            q_plain = A.T @ (A @ pc)
            qr = q_plain + Xw.T @ (Xw @ pc)
            err = np.abs(q - qr).max() / np.abs(qr).max()
            act = np.abs(q - q_plain).max() / np.abs(qr).max()
            print(f'{name} mask_x={mask_x}: m_x {m_x}, err {err:.2e}, term {act:.2e}')
            assert err <= 1e-12, (name, err)
            if Xw.nnz:
                assert act > 1e-9, name                                           # the term did act
            assert np.array_equal(q, fs.solver.normal_apply(pf)[keep_cols]), name   # run to run
        # the assembled operator holds the rows too: the stacked reference, entry for entry
        G = fs.solver.get_csr()
        R = sp.vstack([A, Xw]).tocsr()
        R.sort_indices()
        assert np.array_equal(G.indptr, R.indptr) and np.array_equal(G.indices, R.indices), name
        assert np.abs(G.data - R.data).max() <= 1e-15 * np.abs(R.data).max(), name
    finally:
        fs.close()


@pytest.mark.parametrize('m_x', [1, 63, 64, 65, BLOCK - 1, BLOCK + 1])
def test_normal_operator_with_extra_rows_sizes(gpu_available, m_x):
    rng = np.random.default_rng(100 + m_x)
    _check_operator(_csr(_random_rows(rng, m_x)), rng, f'random{m_x}', mask_x=m_x > 1)


@pytest.mark.parametrize('mask_x', [False, True])
def test_normal_operator_with_extra_rows_special_layouts(gpu_available, mask_x):
    rng = np.random.default_rng(31)
    _check_operator(_csr(_special_rows(rng)), rng, 'special', mask_x)


def _raw_solver(stage):
    """an LSQSolver formed from t64's descriptors after stage(solver) ran on the empty handle"""
    S, kw, keep_cols, w, rhs, keep, A = _base()
    from lssurf_amd.assemble import describe
    gdesc, interp, coords, stencils, npts, fields = describe(S['G_data'], S['Gc'], with_fields=True)
    sv = LSQSolver(0)
    try:
        sv.set_col_map(S['Gc'].col_N, keep_cols)
        m_x = stage(sv)
        sv.set_matrix_stencil(w.size + m_x, S['Gc'].col_N, gdesc, interp, coords, stencils, npts, fields=fields)
        sv.set_column_blocks_affine(*node_column_blocks_affine(S['grids'], keep_cols))
    except Exception:
        sv.close()
        raise
    return sv


def test_a_33_entry_row_is_refused_and_the_staging_stays(gpu_available):
    S, kw, keep_cols, w, rhs, keep, A = _base()
    rng = np.random.default_rng(32)
    z0, dz, removed = _cols()
    kept_dz = np.setdiff1d(dz, removed)
    good = _csr(_random_rows(rng, 70))
    bad = _csr(_random_rows(rng, 5) + [(kept_dz[2000:2033], np.ones(33))])
    # 33 entries of which one is removed, one a zero and two a duplicate pair still pass: ≤ 32 are kept
    fine = _csr([(np.r_[kept_dz[2000:2030], removed[0], kept_dz[2000], kept_dz[2031]], np.r_[np.ones(31), 2., 0.])])

    def stage(sv):
        sv.set_extra_rows(*fine)
        sv.set_extra_rows(*good)
        with pytest.raises(NativeError, match='more than 32'):
            sv.set_extra_rows(*bad)
        return 70

    sv = _raw_solver(stage)
    try:
        G = sv.get_csr()
    finally:
        sv.close()
    R = sp.vstack([_unmasked_A(), _host_X(good, keep_cols, S['Gc'].col_N)]).tocsr()
    R.sort_indices()
    R.eliminate_zeros()
    assert np.array_equal(G.indptr, R.indptr) and np.array_equal(G.indices, R.indices)
    assert np.array_equal(G.data, R.data)


@functools.lru_cache(maxsize=None)
def _unmasked_A():
    sv = _raw_solver(lambda sv: 0)
    try:
        return sv.get_csr()
    finally:
        sv.close()


def test_with_biases_the_two_terms_add(gpu_available):
    S, kw, keep_cols, w, rhs, keep, A = _base()
    rng = np.random.default_rng(33)
    csr = _csr(_random_rows(rng, 200))
    wx = rng.uniform(0.5, 20., 200)
    Xw = sp.diags(wx) @ _host_X(csr, keep_cols, S['Gc'].col_N)
    ids, c = _layouts(keep.size, keep, rng)['mixed']
    fs = _system(csr)
    try:
        fs.solver.set_row_weight(np.r_[w, wx])
        fs.solver.set_row_mask(np.concatenate([keep, np.ones(fs.n_con, bool)]))
        fs.solver.set_data_bias(ids, c)
        ok, why = fs.solver.cg_available(3)
        assert ok, why
        pc = rng.standard_normal(A.shape[1])
        pf = np.zeros(fs.n_full)
        pf[keep_cols] = pc
        q = fs.solver.normal_apply(pf)[keep_cols]
        qr = _host_reduced(A, int(keep.sum()), w[:keep.size][keep], ids[keep], c, pc) + Xw.T @ (Xw @ pc)
        assert np.abs(q - qr).max() <= 1e-12 * np.abs(qr).max()
        assert np.array_equal(q, fs.solver.normal_apply(pf)[keep_cols])
    finally:
        fs.close()


def test_profile_extra_rows_runs_real_iterations(gpu_available):
    """profile_extra_rows: refused without the live state of iterate() and without extra rows (the
    handle goes on iterating); on the live state it runs real steps (the same estimates after 16 as
    plain iterations give) and returns its four documented times, all positive."""
    S, kw, keep_cols, w, rhs, keep, A = _base()
    rng = np.random.default_rng(36)
    csr = _csr(_random_rows(rng, 200))
    wx = rng.uniform(0.5, 20., 200)
    for extra in (True, False):
        fs = _system(csr if extra else None)
        b = np.r_[rhs, np.zeros(200)] if extra else rhs
        try:
            fs.solver.set_row_weight(np.r_[w, wx] if extra else w)
            fs.solver.set_row_mask(np.concatenate([keep, np.ones(fs.n_con, bool)]))
            with pytest.raises(NativeError, match='live state'):
                fs.solver.profile_extra_rows(reps=3)
            if extra:
                prof = _profiler_runs_real_iterations(fs.solver, b, keep.size,
                                                      lambda reps: fs.solver.profile_extra_rows(reps=reps),
                                                      lambda: fs.solver.normal_apply(np.zeros(fs.n_full)))
                assert list(prof) == ['k_xr_fwd', 'k_xr_atq', 'data_fwd', 'node_gather']
                _times_are_positive(prof.values())
            else:
                st = fs.solver.iterate(b, 3, precond=3, method=1, b_rows=keep.size)
                with pytest.raises(NativeError, match='no extra rows'):
                    fs.solver.profile_extra_rows(reps=3)      # a live state, no extra rows
                assert fs.solver.iterate(b, 2, precond=3, method=1, b_rows=keep.size)['iters'] == st['iters'] + 2
        finally:
            fs.close()


def test_cleared_staging_restores_every_bit(gpu_available):
    S, kw, keep_cols, w, rhs, keep, A = _base()
    rng = np.random.default_rng(34)
    csr = _csr(_random_rows(rng, 100))

    def staged_then_cleared(sv):
        sv.set_extra_rows(*csr)
        sv.set_extra_rows(None, None, None)
        return 0

    res = []
    for stage in (lambda sv: 0, staged_then_cleared):
        sv = _raw_solver(stage)
        try:
            sv.set_row_weight(w)
            sv.set_row_mask(np.concatenate([keep, np.ones(w.size - keep.size, bool)]))
            x, st = sv.solve(rhs, precond=3, method=1, b_rows=keep.size, **TOL)
            pf = np.zeros(S['Gc'].col_N)
            pf[keep_cols] = np.random.default_rng(35).standard_normal(keep_cols.size)
            res.append((x, sv.normal_apply(pf), st['iters'], st['method']))
        finally:
            sv.close()
    assert res[0][3] == res[1][3] == 1
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2]


@functools.lru_cache(maxsize=None)
def _edge_objects():
    g = golden('sys_prior_edge.npz')
    kw = prior_kwargs(g)
    S = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, **kw)
    keep_cols = reference_epoch_keep_cols(S['G_data'].col_N, S['grids']['dz'], kw['reference_epoch'])
    w = 1. / np.concatenate((S['Ed'], S['Ec']))
    return g, S, keep_cols, w, S['rhs']


def test_recorded_tile_edge_system_solves(gpu_available):
    g, S, keep_cols, w, rhs = _edge_objects()
    xs, n_prior = g['x'], int(g['n_prior'])
    assert np.any(rhs[-n_prior:] != 0)
    fs = FitSystem(S['G_data'], S['Gc'], keep_cols, S['Gc'].col_N, grids=S['grids'], extra_ops=S['prior_ops'])
    keep = np.ones(fs.n_data, bool)
    try:
        assert fs.formation == 'stencil' and fs.n_extra == n_prior   # not formed by COO
        fs.b_rows = fs.n_data                                         # the library uploads the priors' b itself
        runs = {}
        for name, opts in (('bj', dict(precond=3, method=1)), ('jacobi', dict(precond=1, method=1)),
                           ('lsqr', dict(precond=3, method=0, op=1))):
            x = fs.solve(w, keep, rhs, maxit=200000, **opts, **TOL)
            st = dict(fs.stats)
            err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
            print(f'{name}: method {st["method"]}, {st["iters"]} iterations, err {err:.2e}')
            assert st['method'] == opts['method'] and st['istop'] in (1, 2), (name, st)
            assert err <= REL and np.max(np.abs(x - xs)) <= ABS, (name, err)
            runs[name] = x
        x2 = fs.solve(w, keep, rhs, maxit=200000, precond=3, method=1, **TOL)
        assert np.array_equal(fs.solve(w, keep, rhs, maxit=200000, precond=3, method=1, **TOL), x2)   # two runs
        # warm start from a perturbed x
        x0 = runs['bj'] * (1 + 1e-3 * np.random.default_rng(36).standard_normal(xs.size))
        xw = fs.solve(w, keep, rhs, x0=x0, maxit=200000, precond=3, method=1, **TOL)
        assert np.linalg.norm(xw - xs) / np.linalg.norm(xs) <= REL and np.max(np.abs(xw - xs)) <= ABS
        xj = fs.solve(w, keep, rhs, x0=x0, maxit=200000, precond=1, method=1, **TOL)
        assert np.linalg.norm(xj - xs) / np.linalg.norm(xs) <= REL
        # multigrid and the structured LSQR operator are refused, with the reason
        with pytest.raises(NativeError, match='multigrid'):
            fs.solve(w, keep, rhs, precond=4, method=1, **TOL)
        ok, why = fs.solver.cg_available(4)
        assert not ok and 'multigrid' in why
        with pytest.raises(NativeError, match='assembled'):
            fs.solve(w, keep, rhs, precond=3, method=0, op=0, **TOL)
        assert not fs.multigrid_available(w)
        info = fs.solver.extra_rows_info()
        assert info['m_x'] == n_prior and info['step_bytes'] > 0 and info['device_bytes'] > 0
    finally:
        fs.close()


def _frame_priors(sigma):
    """node-coincident priors: the dz nodes of a 3-node edge frame of t64, every non-reference
    epoch: rows (1 at the node, −1 at the node's reference-epoch column), weights 1/sigma, priors 0.1·N(0,1)"""
    S, kw = _base()[:2]
    gd = S['grids']['dz']
    ny, nx, nt = gd.shape
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing='ij')
    frame = (yy < 3) | (yy >= ny - 3) | (xx < 3) | (xx >= nx - 3)
    ref = kw['reference_epoch']
    rows = []
    for y, x in zip(yy[frame], xx[frame]):
        for t in range(nt):
            if t != ref:
                rows.append(([gd.col_0 + np.ravel_multi_index((y, x, t), gd.shape),
                              gd.col_0 + np.ravel_multi_index((y, x, ref), gd.shape)], [1., -1.]))
    n = len(rows)
    return _csr(rows), np.full(n, 1. / sigma), 0.1 * np.random.default_rng(37).standard_normal(n)


def test_block_factors_carry_the_term(gpu_available):
    """These rows add a block-diagonal PSD E to both N and M: M + E ≥ M contracts
    M^{-1/2}(N − M)M^{-1/2}, so the preconditioned spectrum's bound cannot widen, while leaving E out of
    the factors would put eigenvalues of 1e4 and above on 8 052 directions.  Host CGNR with factors of
    the full A (oracle.cpu.cgnr_bj, atol 1e-12): 601 iterations without priors, 348 with σ = 1e-4.
    The slack of 2 is test_gpu_block_tab.py's between equivalent factorizations."""
    S, kw, keep_cols, w, rhs, keep, A = _base()
    csr, wx, prior = _frame_priors(1e-4)
    assert wx.size == 8052
    every = np.ones(keep.size, bool)
    fs = _system()
    try:
        fs.b_rows = fs.n_data
        fs.solve(w, every, rhs, precond=3, method=1, maxit=200000, **TOL)
        it_plain = fs.stats['iters']
    finally:
        fs.close()
    fs = _system(csr)
    try:
        fs.b_rows = fs.n_data
        W, b = np.r_[w, wx], np.r_[rhs, prior]
        x = fs.solve(W, every, b, precond=3, method=1, maxit=200000, **TOL)
        st = dict(fs.stats)
        assert st['method'] == 1 and st['istop'] in (1, 2), st
        print(f'block-Jacobi iterations: {it_plain} without priors, {st["iters"]} with')
        assert st['iters'] <= it_plain + 2
        # once more with the full CSR formed: the factors come from the merge over GT
        fs.solver.get_csr()
        xf = fs.solve(W, every, b, precond=3, method=1, maxit=200000, **TOL)
        assert abs(fs.stats['iters'] - st['iters']) <= 2
        assert np.linalg.norm(xf - x) / np.linalg.norm(x) <= REL
    finally:
        fs.close()


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    ok = np.isfinite(b)
    return np.linalg.norm(a[ok] - b[ok]) / max(np.linalg.norm(b[ok]), 1e-300)


@pytest.mark.parametrize('extra, method', [(dict(lsq_method='cgnr', lsq_precond=3), 1), (dict(), 0)])
@pytest.mark.parametrize('name', ['prior_edge', 'prior_dz'])
def test_smooth_fit_with_priors_matches_reference(gpu_available, name, extra, method):
    g = golden(f'sys_{name}.npz')
    S = LS.smooth_fit(data=golden_points(g), **prior_kwargs(g), **extra)
    d, m = S['data'], S['m']
    assert int(np.sum(d.three_sigma_edit != g['data_three_sigma_edit'].astype(bool))) == 0
    assert _rel(d.sigma_extra, g['data_sigma_extra']) < 1e-5
    assert _rel(m['z0'].z0, g['z0']) < 1e-6
    assert _rel(m['dz'].dz, g['dz']) < 1e-6
    assert _rel(d.z_est, g['data_z_est']) < 1e-6
    assert np.array_equal(S['valid_data'], g['valid_data'])
    assert S['timing']['lsq_last']['method'] == method
    assert S['timing']['formation'] == 'stencil' and S['timing']['extra_rows'] == int(g['n_prior'])


def test_rows_that_keep_no_entry_still_count_their_b(gpu_available):
    """Extra rows whose entries all fall away (removed columns, an explicit zero) change no x, but
    their b is part of ‖b‖ and of the residual: CGNR on the lazily formed system and LSQR on the
    assembled operator must report the same r1norm, ‖W_x b_x‖² above the plain system's.
    The three r1norm are f64 recurrences of solves run to atol = btol = 1e-12, compared at the
    project's REL 1e-6; the term under test is some percent of ‖r‖² (printed), so leaving it out of
    either method misses the bound by four orders of magnitude."""
    S, kw, keep_cols, w, rhs, keep, A = _base()
    z0, dz, removed = _cols()
    csr = _csr([(removed[:3], [1., 2., 3.]), ([int(np.setdiff1d(dz, removed)[3])], [0.0]), (removed[5:6], [4.])])
    wx, bx = np.array([2., 3., 0.5]), np.array([5., -7., 11.])
    extra2 = float(np.sum((wx * bx) ** 2))
    plain = _system()
    try:
        plain.solve(w, keep, rhs, precond=3, method=1, **TOL)
        r_plain = plain.stats['r1norm']
    finally:
        plain.close()
    fs = _system(csr)
    try:
        assert fs.formation == 'stencil' and fs.n_extra == 3
        wa, ba = np.r_[w, wx], np.r_[rhs, bx]
        fs.b_rows = fs.n_data   # the library uploads the extra rows' b itself
        xc = fs.solve(wa, keep, ba, precond=3, method=1, **TOL)
        rc, mc = fs.stats['r1norm'], fs.stats['method']
        xl = fs.solve(wa, keep, ba, precond=3, method=0, op=1, maxit=200000, **TOL)
        rl, ml = fs.stats['r1norm'], fs.stats['method']
    finally:
        fs.close()
    print(f'r1norm: plain {r_plain:.12e}, CGNR {rc:.12e}, LSQR {rl:.12e}, extra {np.sqrt(extra2):.6e}')
    assert (mc, ml) == (1, 0)
    assert np.linalg.norm(xc - xl) <= REL * np.linalg.norm(xl) and np.max(np.abs(xc - xl)) <= ABS
    assert extra2 > 1e-2 * rc ** 2
    assert abs(rc - rl) <= REL * rl
    assert abs(rc ** 2 - (r_plain ** 2 + extra2)) <= REL * rc ** 2


def test_staged_rows_are_not_dropped_by_the_coo_formation(gpu_available):
    """lsq_set_matrix_coo takes no extra rows: with rows staged it refuses (and names the way out)
    instead of forming a system without them; after clearing the staging it forms."""
    rng = np.random.default_rng(37)
    sv = LSQSolver(0)
    try:
        sv.set_extra_rows(*_csr([([0, 3], [1., -1.]), ([2], [2.])]))
        r, c, v = np.array([0, 1, 2, 3]), np.array([0, 1, 2, 3]), rng.standard_normal(4)
        with pytest.raises(NativeError, match='staged'):
            sv.set_matrix_coo(4, 4, r, c, v)
        sv.set_extra_rows(None, None, None)
        sv.set_matrix_coo(4, 4, r, c, v)
        assert sv.shape()[:2] == (4, 4)
    finally:
        sv.close()


def _biased_points(g):
    """the tile-edge fixture's points with a three-valued sensor and a 0.3 m offset per sensor"""
    D = golden_points(g)
    sensor = (np.arange(D.size) % 3).astype(float)
    D.assign(sensor=sensor, sigma_corr=np.full(D.size, 0.5))
    D.z[:] = D.z + 0.3 * sensor
    return D


@pytest.mark.parametrize('mode', ['columns', 'auto'])
def test_smooth_fit_priors_with_bias_columns(gpu_available, mode):
    """bias_params with priors runs as a generic (COO-formed) system whose columns hold the biases:
    one linear solve (max_iterations = 1) against the host's sparse normal-equation solve of the same
    weighted system (cond(A) ≈ 9e2, so that reference is good to ~1e-12).  'auto' with a dense
    limit that would make it eliminate warns that it takes 'columns' instead."""
    import warnings
    import scipy.sparse.linalg as spl
    g = golden('sys_prior_edge.npz')
    kw = dict(prior_kwargs(g), bias_params=['sensor'], max_iterations=1)
    O = LS.smooth_fit(data=_biased_points(g), return_fit_objects=True, lsq_bias='columns', **kw)
    Gd, Gc = O['G_data'], O['Gc']
    keep_cols = reference_epoch_keep_cols(Gd.col_N, O['grids']['dz'], kw['reference_epoch'])
    w = 1. / np.concatenate((O['Ed'], O['Ec']))
    A = sp.vstack([Gd.toCSR(row_N=Gd.N_eq, col_N=Gc.col_N), Gc.toCSR(row_N=Gc.N_eq, col_N=Gc.col_N)]).tocsr()
    A = (sp.diags(w) @ A[:, keep_cols]).tocsc()
    x = np.zeros(Gc.col_N)
    x[keep_cols] = spl.spsolve((A.T @ A).tocsc(), A.T @ (w * O['rhs']))
    if mode == 'auto':
        with pytest.warns(RuntimeWarning, match="takes 'columns'"):
            S = LS.smooth_fit(data=_biased_points(g), lsq_bias='auto', lsq_dense_max=0, **kw)
    else:
        with warnings.catch_warnings():   # asked for by name: nothing to warn about
            warnings.filterwarnings('error', message=".*takes 'columns'.*")
            S = LS.smooth_fit(data=_biased_points(g), lsq_bias='columns', **kw)
    assert S['timing']['formation'] == 'coo' and S['timing']['extra_rows'] == 0
    m = S['m']
    cz, cd = Gd.TOC['cols']['z0'], Gd.TOC['cols']['dz']
    assert _rel(m['z0'].z0, x[cz].reshape(m['z0'].z0.shape)) < 1e-6
    assert _rel(m['dz'].dz, x[cd].reshape(m['dz'].dz.shape)) < 1e-6
    assert _rel(S['data'].z_est, Gd.toCSR(row_N=Gd.N_eq, col_N=Gc.col_N) @ x) < 1e-6
    assert _rel(m['bias']['val'], x[-3:]) < 1e-6
