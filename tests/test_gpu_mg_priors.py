"""The multigrid preconditioner (precond 4) with extra rows lumped into its coarse levels
(lsq_set_extra_rows_lumping; csrc/xr_lump.hpp, k_mg_lump_xr in csrc/mg.inc) and smooth_fit's
lsq_prior_mg on top of it.

Level operators: every level of a handle with lumped extra rows equals the host hierarchy
(tests/mg_host.py) of A', the weighted, kept extra rows (host scipy) put behind the data rows of
get_csr() of a handle that never saw an extra row — so the host lumps them exactly as it lumps data
rows.  Tolerances are those of test_gpu_mg.py (1e-11 operators, 1e-10 symmetry, 1e-8 solves)."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import lssurf_amd as LS
from conftest import golden, golden_points
from lssurf_amd import containers as pc
from lssurf_amd._native import NativeError
from lssurf_amd.constraint_functions import reference_epoch_keep_cols
from lssurf_amd.match_priors import make_prior_op
from lssurf_amd.smooth_fit import FitSystem, _extra_rows_csr
from mg_host import hierarchy
from priors_common import prior_kwargs
from test_gpu_priors import _csr, _random_rows, _rel

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
from prior_step import frame_rows  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = dict(atol=1e-12, btol=1e-12, conlim=1e12)


@functools.lru_cache(maxsize=None)
def _host_of(name):
    """(S, kw, keep_cols): the host objects of a synthetic system (no device)"""
    from lssurf_amd import synthetic
    D, kw = synthetic.points(name)
    S = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw)
    keep_cols = reference_epoch_keep_cols(S['G_data'].col_N, S['grids']['dz'], kw['reference_epoch'])
    keep_cols.flags.writeable = False
    return S, kw, keep_cols


@functools.lru_cache(maxsize=None)
def _base_of(name):
    """(S, kw, keep_cols, w, rhs, keep, A) of a synthetic system, A the weighted, row-selected matrix of a
    handle that never saw an extra row (as test_gpu_priors._base).  Shared, never changed."""
    S, kw, keep_cols = _host_of(name)
    w = 1. / np.concatenate((S['Ed'], S['Ec']))
    rhs = np.zeros(w.size)
    rhs[:S['data'].size] = S['data'].z
    keep = np.random.default_rng(22).random(S['data'].size) > 0.2
    fs = FitSystem(S['G_data'], S['Gc'], keep_cols, S['Gc'].col_N, grids=S['grids'])
    try:
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(np.concatenate([keep, np.ones(fs.n_con, bool)]))
        A = fs.solver.get_csr()
    finally:
        fs.close()
    for a in (w, rhs, keep):
        a.flags.writeable = False
    return S, kw, keep_cols, w, rhs, keep, A


def _system(name, csr, lump=True):
    S, kw, keep_cols = _host_of(name)
    return FitSystem(S['G_data'], S['Gc'], keep_cols, S['Gc'].col_N, grids=S['grids'], extra_csr=csr, extra_mg=lump)


def _rows_frame(name):
    """(a) the node-aligned frame of tools/prior_step.py scaled to the grid (t64: 49-node tile, 2-node strips)"""
    S, kw = _host_of(name)[:2]
    gd = S['grids']['dz']
    tile = 49 if name == 't64' else min(gd.shape[:2]) - 4
    return frame_rows(gd, kw['reference_epoch'], tile, 2)


def _rows_interp(name, n=700):
    """(b) make_prior_op on the points of a saved grid shifted by 0.37 of the spacing in x and y, epochs
    between the fit's: 8 to 12 entries per row, points in the last cell row and column, t in the first and
    the last interval among them"""
    S, kw = _host_of(name)[:2]
    gd = S['grids']['dz']
    y, x, t = (np.asarray(c, float) for c in gd.ctrs)
    dy, dx = y[1] - y[0], x[1] - x[0]
    rng = np.random.default_rng(41)
    ys = (y[:-1] + 0.37 * dy)[::max(1, (y.size - 1) // 12)]
    xs = (x[:-1] + 0.37 * dx)[::max(1, (x.size - 1) // 12)]
    ys, xs = np.unique(np.r_[ys, y[-2] + 0.37 * dy]), np.unique(np.r_[xs, x[-2] + 0.37 * dx])   # the last cells
    ts = t[:-1] + rng.uniform(0.2, 0.8, t.size - 1) * np.diff(t)                                  # every interval
    Y, X, T = (a.ravel() for a in np.meshgrid(ys, xs, ts, indexing='ij'))
    pick = rng.permutation(Y.size)[:n]
    pts = pc.data().from_dict({'y': Y[pick], 'x': X[pick], 't': T[pick], 'dz': np.zeros(pick.size),
                               'sigma_dz': np.ones(pick.size)})
    op = make_prior_op(S['grids'], pts, 'shifted', ref_time=float(t[kw['reference_epoch']]))
    csr = _extra_rows_csr([op])
    keep_cols = _host_of(name)[2]
    X = sp.csr_matrix((csr[2].copy(), csr[1].copy(), csr[0].copy()), shape=(csr[0].size - 1, S['Gc'].col_N))
    X.sum_duplicates()
    X.eliminate_zeros()
    per_row, kept = np.diff(X.indptr), np.diff(X[:, keep_cols].tocsr().indptr)
    assert per_row.min() >= 8 and per_row.max() <= 12, (per_row.min(), per_row.max())    # as staged
    assert kept.min() >= 4 and kept.max() <= 8, (kept.min(), kept.max())                  # as the device keeps them
    return csr


def _rows_edge(name):
    """(c) 300 rows on one fine node (the wave-per-node path), rows whose every entry is in a removed
    column, a row with a z0 and a dz part (τ_z = 1), single-epoch rows at the last epoch"""
    S, kw = _host_of(name)[:2]
    gz, gd = S['grids']['z0'], S['grids']['dz']
    ny, nx, nt = gd.shape
    ref = kw['reference_epoch']
    rng = np.random.default_rng(42)
    col = lambda yy, xx, tt: int(gd.col_0 + np.ravel_multi_index((yy, xx, tt), gd.shape))   # noqa: E731
    colz = lambda yy, xx: int(gz.col_0 + np.ravel_multi_index((yy, xx), gz.shape))          # noqa: E731
    live = [t for t in range(nt) if t != ref]
    rows = []
    hy, hx = ny // 2 + 1 - (ny // 2) % 2, nx // 2 + 1 - (nx // 2) % 2       # an odd-odd node: four parents
    for k in range(300):
        t = live[k % len(live)]
        rows.append(([col(hy, hx, t), col(hy, hx, ref)], [1., -1.]))
    for k in range(5):
        rows.append(([col(k, k + 1, ref), col(k + 1, k, ref)], [1., -2.]))
    for k in range(6):
        yy, xx, t = int(rng.integers(ny)), int(rng.integers(nx)), int(rng.integers(nt - 1))
        f = float(rng.uniform(0.1, 0.9))
        rows.append(([colz(yy, xx), col(yy, xx, t), col(yy, xx, t + 1)], [1., 1. - f, f]))
    for k in range(7):
        yy, xx = int(rng.integers(ny)), int(rng.integers(nx))
        rows.append(([col(yy, xx, nt - 1 if ref != nt - 1 else nt - 2)], [float(rng.uniform(0.5, 2.))]))
    order = rng.permutation(len(rows))
    return _csr([rows[i] for i in order])


def _stack(*csrs):
    ip = [np.zeros(1, np.int64)]
    for c in csrs:
        ip.append(c[0][1:] + ip[-1][-1])
    return np.concatenate(ip), np.concatenate([c[1] for c in csrs]), np.concatenate([c[2] for c in csrs])


@functools.lru_cache(maxsize=None)
def _rows_all(name):
    return _stack(_rows_frame(name), _rows_interp(name), _rows_edge(name))


def _weights(m_x, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 20., m_x), rng.random(m_x) > 0.25


def _host_rows(name, csr, wx, kx):
    S, kw, keep_cols = _host_of(name)
    X = sp.csr_matrix((csr[2].copy(), csr[1].copy(), csr[0].copy()), shape=(csr[0].size - 1, S['Gc'].col_N))
    X = X[:, keep_cols].tocsr()                      # scipy sums the duplicates
    return (sp.diags(wx[kx]) @ X[kx]).tocsr()


def _set(fs, name, wx, kx):
    S, kw, keep_cols, w, rhs, keep, A = _base_of(name)
    fs.solver.set_row_weight(np.r_[w, wx])
    fs.solver.set_row_mask(np.concatenate([keep, np.ones(fs.n_con - wx.size, bool), kx]))


@pytest.mark.parametrize('name', ['t64', 't15'])
def test_level_operators_with_lumped_rows_match_host(gpu_available, name):
    S, kw, keep_cols, w, rhs, keep, A = _base_of(name)
    csr = _rows_all(name)
    m_x = csr[0].size - 1
    wx, kx = _weights(m_x, 43)
    n_d = int(keep.sum())
    Xw = _host_rows(name, csr, wx, kx)
    A1 = sp.vstack([A[:n_d], Xw, A[n_d:]]).tocsr()
    ny, nx, nt = S['grids']['dz'].shape
    host = hierarchy(A1, n_d + Xw.shape[0], keep_cols, ny, nx, nt)
    plain = hierarchy(A, n_d, keep_cols, ny, nx, nt)
    rng = np.random.default_rng(44)
    fs = _system(name, csr)
    try:
        _set(fs, name, wx, kx)
        ok, why = fs.solver.cg_available(4)
        assert ok, why
        info = fs.solver.extra_rows_mg_info()
        print(name, 'lumped:', info)
        assert 0 < info['rows'] < m_x and info['nodes'] > 0 and info['pass_bytes'] > 0 and info['device_bytes'] > 0
        assert info['nodes'] % 64 != 0
        levels, tref = fs.solver.mg_info()
        assert len(host) == len(levels)
        for l, ((shape, kmask, N), (S0, S1, nf)) in enumerate(zip(host, levels)):
            assert shape == (S0, S1) and nf == kmask.size
            if l == len(levels) - 1:
                break
            for _ in range(2):
                x = np.where(kmask, rng.standard_normal(nf), 0.0)
                y = fs.solver.mg_apply(l, 0, x)
                yr = N @ x
                err = np.abs(y - yr).max() / np.abs(yr).max()
                term = np.abs(yr - plain[l][2] @ x).max() / np.abs(yr).max()
                print(f'{name} level {l}: err {err:.2e}, the rows\' share {term:.2e}')
                assert err <= 1e-11, (l, err)
                assert term > 1e-6, (l, term)          # a hierarchy without the rows misses the bound
                assert np.all(y[~kmask] == 0.0)
            lam = fs.solver.mg_apply(l, 2)
            assert np.isfinite(lam) and lam > 0.5, (l, lam)
    finally:
        fs.close()


def test_vcycle_with_lumped_rows_is_spd_and_follows_the_weights(gpu_available):
    S, kw, keep_cols, w, rhs, keep, A = _base_of('t64')
    csr = _rows_all('t64')
    m_x = csr[0].size - 1
    wx, kx = _weights(m_x, 45)
    rng = np.random.default_rng(46)
    fs = _system('t64', csr)
    try:
        _set(fs, 't64', wx, kx)
        ok, why = fs.solver.cg_available(4)
        assert ok, why
        nf = fs.n_full
        kmask = np.zeros(nf, bool)
        kmask[keep_cols] = True
        u = np.where(kmask, rng.standard_normal(nf), 0.0)
        v = np.where(kmask, rng.standard_normal(nf), 0.0)
        Vu, Vv = fs.solver.mg_apply(0, 1, u), fs.solver.mg_apply(0, 1, v)
        Vu2 = fs.solver.mg_apply(0, 1, u)
        fs.solver.set_row_weight(np.r_[w, 3. * wx])
        Vu3 = fs.solver.mg_apply(0, 1, u)
    finally:
        fs.close()
    assert np.array_equal(Vu, Vu2)
    assert np.all(Vu[~kmask] == 0.0)
    a, b = v @ Vu, u @ Vv
    assert abs(a - b) <= 1e-10 * (abs(a) + abs(b)), (a, b)
    assert u @ Vu > 0 and v @ Vv > 0
    assert np.abs(Vu3 - Vu).max() > 1e-6 * np.abs(Vu).max()


def test_solves_with_lumped_frame_priors(gpu_available):
    """Frame (a), σ = 0.01, priors N(0, 0.05), every row kept.  CPU prototype
    (tools/mg_prior_proto.py): 36 multigrid iterations with and without the priors, 468 block-Jacobi
    iterations, and 780 for a hierarchy whose coarse levels miss the priors."""
    S, kw, keep_cols, w, rhs, keep, A = _base_of('t64')
    csr = _rows_frame('t64')
    m_x = csr[0].size - 1
    assert m_x == 4136
    wx = np.full(m_x, 1. / 0.01)
    prior = 0.05 * np.random.default_rng(47).standard_normal(m_x)
    every = np.ones(keep.size, bool)
    W, b = np.r_[w, wx], np.r_[rhs, prior]
    plain = FitSystem(S['G_data'], S['Gc'], keep_cols, S['Gc'].col_N, grids=S['grids'])
    try:
        plain.b_rows = plain.n_data
        plain.solve(w, every, rhs, precond=4, method=1, **TOL)
        it_plain = plain.stats['iters']
    finally:
        plain.close()
    fs = _system('t64', csr)
    try:
        fs.b_rows = fs.n_data
        xb = fs.solve(W, every, b, precond=3, method=1, maxit=200000, **TOL)
        it_bj = fs.stats['iters']
        xm = fs.solve(W, every, b, precond=4, method=1, **TOL)
        st = dict(fs.stats)
        xm2 = fs.solve(W, every, b, precond=4, method=1, **TOL)
        xw = fs.solve(W, every, b, x0=xm * (1 + 1e-4), precond=4, method=1, **TOL)
        it_warm = fs.stats['iters']
    finally:
        fs.close()
    print(f'iterations: multigrid {st["iters"]} (warm {it_warm}), without priors {it_plain}, block-Jacobi {it_bj}')
    assert st['method'] == 1 and st['istop'] in (1, 2), st
    assert np.linalg.norm(xm - xb) / np.linalg.norm(xb) <= 1e-8
    assert np.array_equal(xm, xm2)
    assert np.linalg.norm(xw - xb) / np.linalg.norm(xb) <= 1e-8
    assert it_warm <= st['iters']
    assert st['iters'] * 5 <= it_bj, (st['iters'], it_bj)
    assert st['iters'] <= 2 * it_plain, (st['iters'], it_plain)


def test_rows_that_cannot_be_lumped_are_refused_with_the_reason(gpu_available):
    S, kw, keep_cols, w, rhs, keep, A = _base_of('t64')
    rng = np.random.default_rng(48)
    csr = _csr(_random_rows(rng, 70))
    wx = rng.uniform(0.5, 20., 70)
    fs = _system('t64', csr)
    try:
        fs.b_rows = fs.n_data
        fs.solver.set_row_weight(np.r_[w, wx])
        fs.solver.set_row_mask(np.concatenate([keep, np.ones(fs.n_con, bool)]))
        ok, why = fs.solver.cg_available(4)
        assert not ok and 'cannot be lumped' in why and 'extra row' in why, why
        with pytest.raises(NativeError, match='cannot be lumped'):
            fs.solver.solve(np.r_[rhs, np.zeros(70)], precond=4, method=1, **TOL)
        with pytest.warns(RuntimeWarning, match='cannot be lumped'):
            assert not fs.multigrid_available()
        assert fs.solver.extra_rows_mg_info()['rows'] == 0
        x, st = fs.solver.solve(np.r_[rhs, np.zeros(70)], precond=3, method=1, b_rows=fs.n_data, **TOL)
        assert st['method'] == 1 and st['istop'] in (1, 2), st
    finally:
        fs.close()
    # without the request the refusal is the one from before lumping existed
    fs = _system('t64', _rows_frame('t64'), lump=False)
    try:
        ok, why = fs.solver.cg_available(4)
        assert not ok and 'does not carry extra rows' in why, why
        assert not fs.multigrid_available()
    finally:
        fs.close()


def test_z0_refined_hierarchy_reports_its_reason(gpu_available):
    """test_gpu_mg.py::_mixed_system's t64z (z0 on a 2× refinement of the dz lattice) with frame rows"""
    from lssurf_amd import synthetic
    D, kw = synthetic.points('t64z')
    S = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw)
    keep_cols = reference_epoch_keep_cols(S['G_data'].col_N, S['grids']['dz'], kw['reference_epoch'])
    csr = frame_rows(S['grids']['dz'], kw['reference_epoch'], 49, 2)
    fs = FitSystem(S['G_data'], S['Gc'], keep_cols, S['Gc'].col_N, grids=S['grids'], extra_csr=csr, extra_mg=True)
    try:
        w = 1. / np.concatenate((S['Ed'], S['Ec']))
        fs.solver.set_row_weight(np.r_[w, np.full(csr[0].size - 1, 10.)])
        ok, why = fs.solver.cg_available(4)
        print('t64z:', ok, why)
        assert not ok and 'z0-refined' in why, why
        assert fs.solver.extra_rows_mg_info()['rows'] == 0
    finally:
        fs.close()


@pytest.mark.parametrize('name', ['prior_edge', 'prior_dz'])
def test_smooth_fit_prior_mg_matches_reference(gpu_available, name):
    g = golden(f'sys_{name}.npz')
    with warnings.catch_warnings():
        warnings.filterwarnings('error', message='.*multigrid does not carry.*')
        S = LS.smooth_fit(data=golden_points(g), lsq_prior_mg=True, lsq_dense_max=0, **prior_kwargs(g))
    d, m = S['data'], S['m']
    assert S['timing']['prior_mg'] is True and S['timing']['lsq_last']['precond'] == 4
    assert S['timing']['formation'] == 'stencil' and S['timing']['extra_rows'] == int(g['n_prior'])
    assert int(np.sum(d.three_sigma_edit != g['data_three_sigma_edit'].astype(bool))) == 0
    assert _rel(d.sigma_extra, g['data_sigma_extra']) < 1e-5
    assert _rel(m['z0'].z0, g['z0']) < 1e-6
    assert _rel(m['dz'].dz, g['dz']) < 1e-6
    assert _rel(d.z_est, g['data_z_est']) < 1e-6
    assert np.array_equal(S['valid_data'], g['valid_data'])
