"""CGNR at 16 to 64 epochs on matrix-free data rows (lsq_set_cg_tile_dmf, FitSystem(tile_dmf=True),
smooth_fit(lsq_tile_eliminate=True)): tile and chunk mode run the step in column mode's order (NORMAL
without the stored ATd rows, k_cg_dmf_ad, the elimination, the node gather — k_cg_dmf_atq_long above 16
epochs), so data biases, slopes and sensor grids are eliminated there as they are below 16 epochs.

Frames: tile_elim_host.points — cgnr_host.ksweep_points with 2 600 points ((9, 11): 1 200), twelve of
them on the upper bounds of y, x and t.  (7, 70): two x strips, the second 6 nodes wide, rows no multiple
of ty; (5, 200): strips clear of both edges; (9, 11): dense-solvable.  Epochs 16 (k_cg_dmf_atq<16> in
the new order), 17, 19 (tile mode), 20 (unequal chunks), 41 and 64 (chunk mode, the cap).

References and bounds are those of the tests these extend: AᵀA p from get_csr() within 1e-12 of max|AᵀA p|
(tests/test_gpu_cgnr.py), the reduced operators' host forms of tests/test_gpu_bias.py, test_gpu_slope.py,
test_gpu_sgrid.py and test_gpu_sgrid_joint.py within 1e-12, oracle.dense.ls_solve_dense of the system with
the eliminated columns written out under DESIGN.md's REL 1e-6 / ABS 1e-4 (biases and slopes 1e-6
relative), smooth_fit against lsq_bias='columns' within 1e-6.  Every case asserts the mode it ran in."""
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import conftest  # noqa: F401
import cgnr_host as H
import lssurf_amd as LS
import tile_elim_host as T
from lssurf_amd._native import NativeError, load
from oracle.dense import ls_solve_dense
from test_gpu_cgnr import ABS, REL, TOL
from test_gpu_cgnr_iterates import ZERO, _open

pytestmark = pytest.mark.gpu
NPTS = {(7, 70): 2600, (5, 200): 2600, (9, 11): 1200}
EPOCHS = (16, 17, 19, 20, 41, 64)
TILE_CASE, CHUNK_CASE = ((7, 70), 17), ((5, 200), 41)


def _host(shape, nt):
    return T.host(shape, NPTS[shape], nt)


def _want(nt):
    return ('tile' if nt < 20 else 'chunk', 'matrix-free')


def _mode(solver, precond=3):
    """(normal_mode, data_rows) of profile_cg; drops the live state, so before the solves"""
    p = solver.profile_cg(reps=1, precond=precond)
    return p['normal_mode'], p['data_rows']


def _kw(nt, on=True):
    return dict(tile_dmf=on, cg_chunks=nt >= 20)


def _full(fs, pc):
    pf = np.zeros(fs.n_full)
    pf[fs.keep_cols] = pc
    return pf


# ---- 1. the plain operator ---------------------------------------------------------------------------
@pytest.mark.parametrize('nt', EPOCHS)
@pytest.mark.parametrize('shape', list(NPTS))
def test_plain_operator(gpu_available, shape, nt):
    """normal_apply on matrix-free data rows in tile / chunk mode against AᵀA p from get_csr(), under a
    row mask and non-uniform weights, bit-identical run to run: k_cg_dmf_atq_long (17 and more epochs)
    and k_cg_normal / k_cg_normal_chunk without ATd."""
    h = _host(shape, nt)
    w, mask = H.mask_and_weights(h)
    rng = np.random.default_rng(7)
    fs = _open(h, w, mask, **_kw(nt))
    try:
        assert _mode(fs.solver) == _want(nt)
        qs = []
        ps = [rng.standard_normal(h.keep_cols.size) for _ in range(2)]
        for p in ps:
            q = fs.solver.normal_apply(_full(fs, p))
            assert np.array_equal(q, fs.solver.normal_apply(_full(fs, p)))   # run to run
            qs.append(q[fs.keep_cols])
        A = fs.solver.get_csr()
    finally:
        fs.close()
    for p, q in zip(ps, qs):
        qr = A.T @ (A @ p)
        err = np.abs(q - qr).max() / np.abs(qr).max()
        print(f'{shape} x {nt}: operator {err:.2e}')
        assert err <= 1e-12, err


# ---- 2. the reduced operators ------------------------------------------------------------------------
def _reduced_frame(shape, nt, seed):
    """an open handle under a data-row mask and h's weights, A = get_csr(), one random p and q = N p"""
    h = _host(shape, nt)
    rng = np.random.default_rng(seed)
    keep = rng.random(h.n_data) > 0.2
    fs = _open(h, h.w, np.concatenate([keep, np.ones(h.w.size - h.n_data, bool)]), **_kw(nt))
    try:
        assert _mode(fs.solver) == _want(nt)
        A = fs.solver.get_csr()          # before anything is set: the grid operator
        pc = rng.standard_normal(A.shape[1])
        q_plain = fs.solver.normal_apply(_full(fs, pc))[fs.keep_cols]
    except BaseException:
        fs.close()
        raise
    return h, fs, rng, keep, A, pc, q_plain


def _check(tag, fs, pc, qr, q_base, limit=1e-12, acts=True):
    ok, why = fs.solver.cg_available(1)
    assert ok, (tag, why)
    q = fs.solver.normal_apply(_full(fs, pc))[fs.keep_cols]
    err = np.abs(q - qr).max() / np.abs(qr).max()
    acted = np.abs(q - q_base).max() / np.abs(qr).max()
    print(f'{tag}: err {err:.2e} (limit {limit:.0e}), the eliminated columns change q by {acted:.2e}')
    assert err <= limit, (tag, err)
    if acts:
        assert acted > 1e-9, (tag, acted)          # the correction is not zero
    assert np.array_equal(q, fs.solver.normal_apply(_full(fs, pc))[fs.keep_cols]), tag   # run to run
    return q


@pytest.mark.parametrize('shape, nt', [TILE_CASE, CHUNK_CASE])
def test_reduced_operator_with_biases(gpu_available, shape, nt):
    from test_gpu_bias import _host_reduced, _layouts
    h, fs, rng, keep, A, pc, q_plain = _reduced_frame(shape, nt, 11)
    try:
        Wk = h.w[:h.n_data][keep]
        layouts = _layouts(h.n_data, keep, rng)
        assert list(layouts) == ['one', 'each', 'mixed', 'masked_id', 'empty_id']
        for name, (ids, c) in layouts.items():
            fs.solver.set_data_bias(ids, c)
            qr = _host_reduced(A, int(keep.sum()), Wk, ids[keep], c, pc)
            _check(f'{shape} x {nt} bias {name}', fs, pc, qr, q_plain)
        assert _mode(fs.solver) == _want(nt)
    finally:
        fs.close()


@pytest.mark.parametrize('shape, nt', [TILE_CASE, CHUNK_CASE])
def test_reduced_operator_with_slopes(gpu_available, shape, nt):
    from test_gpu_slope import _host_reduced, _layouts
    h, fs, rng, keep, A, pc, q_plain = _reduced_frame(shape, nt, 21)
    try:
        n_kept, Wk = int(keep.sum()), h.w[:h.n_data][keep]
        layouts = _layouts(h.n_data, keep, rng)
        for name in ('sizes', 'masked_group', 'empty_group', 'many_ids'):
            ids, c, grp, u, cs = layouts[name]
            for with_bias in ((True, False) if name == 'sizes' else (True,)):
                if with_bias:
                    fs.solver.set_data_bias(ids, c)
                    q_base = fs.solver.normal_apply(_full(fs, pc))[fs.keep_cols]
                else:
                    fs.solver.set_data_bias(None, None)
                    q_base = q_plain
                fs.solver.set_data_slope(grp, u, cs)
                qr, conds = _host_reduced(A, n_kept, Wk, ids[keep] if with_bias else None, c if with_bias else None,
                                          grp[keep], u[keep], cs, pc)
                print(f'{name}: max cond(G) {max(conds):.2e}')
                _check(f'{shape} x {nt} slope {name} {"biases" if with_bias else "nb=0"}', fs, pc, qr, q_base)
    finally:
        fs.close()


def test_reduced_operator_with_sensor_grids(gpu_available):
    from test_gpu_sgrid import _host_reduced, _layouts
    shape, nt = TILE_CASE
    h, fs, rng, keep, A, pc, q_plain = _reduced_frame(shape, nt, 31)
    try:
        n_kept, Wk = int(keep.sum()), h.w[:h.n_data][keep]
        layouts = _layouts(h.n_data, keep, rng)
        for name in ('sizes', 'counts', 'masked_grid', 'empty_grid'):
            fs.solver.set_sensor_grids(*layouts[name])
            qr, conds = _host_reduced(A, n_kept, Wk, keep, layouts[name], pc)
            print(f'{name}: max cond(M_s) {max(conds):.2e}')
            _check(f'{shape} x {nt} sgrid {name}', fs, pc, qr, q_plain)
    finally:
        fs.close()


def test_reduced_operator_with_joint_sensor_grids(gpu_available):
    from test_gpu_sgrid_joint import CLEAR, _c, _host_blocks, _host_reduced, _joint_layouts, _set_bias
    shape, nt = CHUNK_CASE
    h, fs, rng, keep, A, pc, q_plain = _reduced_frame(shape, nt, 41)
    try:
        n_kept, Wk = int(keep.sum()), h.w[:h.n_data][keep]
        layouts = _joint_layouts('t64', h.n_data, keep, rng)
        for name in ('sizes', 'cap', 'loose', 'masked_id', 'one_slope'):
            layout, bias = layouts[name]
            cb, cg = _c(bias, h.w, h.n_data)
            _set_bias(fs, bias, cb, cg)
            q_bs = fs.solver.normal_apply(_full(fs, pc))[fs.keep_cols]      # biases and slopes, no grids
            fs.solver.set_sensor_grids(*layout, joint=True)
            ZW, M, lab = _host_blocks(layout, bias, keep, Wk, cb, cg)
            qr, conds = _host_reduced(A, n_kept, ZW, M, lab, pc)
            print(f'{name}: max cond {max(conds):.2e}')
            _check(f'{shape} x {nt} joint {name}', fs, pc, qr, q_bs)
            fs.solver.set_sensor_grids(*CLEAR)
            fs.solver.set_data_bias(None, None)
    finally:
        fs.close()


# ---- 3. converged solves -----------------------------------------------------------------------------
DENSE = (9, 11)


def _solve_layout(h, with_slopes):
    """5 bias IDs (+ 2 slope groups the IDs nest in), two masks and re-weighted data rows"""
    from test_gpu_slope import _deal, _ids_nested
    rng = np.random.default_rng(51 + with_slopes)
    n = h.n_data
    keep1 = rng.random(n) > 0.1
    keep2 = keep1 & (rng.random(n) > 0.05)
    w = h.w.copy()
    w[:n] *= rng.uniform(0.5, 2, n)
    if with_slopes:
        grp = _deal(n, [300, 200], rng)
        ids, nb = _ids_nested(grp, 2, [2, 1], 2, rng)
        slope = (grp, rng.standard_normal((n, 2)), rng.uniform(1., 5., (2, 2)))
    else:
        ids, nb, slope = rng.integers(0, 5, n).astype(np.int32), 5, None
    return w, (keep1, keep2), ids, rng.uniform(1., 30., nb), slope


@pytest.mark.parametrize('with_slopes', [False, True], ids=['biases', 'biases+slopes'])
@pytest.mark.parametrize('nt', [16, 19, 28, 64])
def test_converged_solves_reach_the_dense_oracle(gpu_available, nt, with_slopes):
    """Cold start, and warm start after a mask change, with block-Jacobi and Jacobi, against the dense
    oracle of the system with the bias (and slope) columns written out."""
    h = _host(DENSE, nt)
    w, keeps, ids, c, slope = _solve_layout(h, with_slopes)
    exact = [ls_solve_dense(*T.written_out(h, w, k, ids, c, slope)[:2]) for k in keeps]
    ng = h.keep_cols.size
    fs = h.fit_system(bias=(ids, c) + ((slope,) if with_slopes else ()), **_kw(nt))
    try:
        assert fs.formation == 'stencil' and fs.has_blocks
        fs.solver.set_row_weight(w)
        assert _mode(fs.solver) == _want(nt)
        for precond in (3, 1):
            x1 = None
            for keep, xs, start in zip(keeps, exact, ('cold', 'warm')):
                x = fs.solve(w, keep, h.rhs, x0=x1, precond=precond, method=1, maxit=400000, **TOL)
                st, b = fs.stats, fs.solver.data_bias()
                assert st['method'] == 1 and st['istop'] in (1, 2), (precond, start, st)
                eg = np.linalg.norm(x - xs[:ng]) / np.linalg.norm(xs[:ng])
                eb = np.linalg.norm(b - xs[ng:ng + c.size]) / np.linalg.norm(xs[ng:ng + c.size])
                print(f'nt {nt} precond {precond} {start}: {st["iters"]} iterations, grid {eg:.2e} '
                      f'(abs {np.max(np.abs(x - xs[:ng])):.2e}), biases {eb:.2e}')
                assert eg <= REL and np.max(np.abs(x - xs[:ng])) <= ABS, (precond, start, eg)
                assert eb <= 1e-6, (precond, start, eb)
                if with_slopes:
                    gam = fs.solver.data_slope().ravel()
                    es = np.linalg.norm(gam - xs[ng + c.size:]) / np.linalg.norm(xs[ng + c.size:])
                    print(f'   slopes {es:.2e}')
                    assert es <= 1e-6, (precond, start, es)
                assert np.any(b != 0)
                x1 = x
    finally:
        fs.close()


# ---- 3b. step mechanics: captured graphs, the profilers' stage marks, the byte model ---------------------
@pytest.mark.parametrize('shape, nt', [TILE_CASE, CHUNK_CASE])
def test_graph_replay_and_profilers_with_biases_and_slopes(gpu_available, shape, nt):
    """With biases and slopes set: eager launches and captured graphs give the same x bit for bit; profile_cg
    and profile_data_slope time real iterations (the run ends where plain iterations end) in column mode's
    order, with positive times at every stage mark; the byte model is the one iterate() reports, its normal
    share tile mode's 32 B per column (chunk mode: more, by the halos) without the stored rows' terms."""
    from test_gpu_cgnr import _profiler_runs_real_iterations, _times_are_positive
    from test_gpu_slope import _layouts
    h = _host(shape, nt)
    rng = np.random.default_rng(81)
    keep = rng.random(h.n_data) > 0.1
    ids, c, grp, u, cs = _layouts(h.n_data, keep, rng)['sizes']
    fs = _open(h, h.w, np.concatenate([keep, np.ones(h.w.size - h.n_data, bool)]), **_kw(nt))
    try:
        plain = fs.solver.iterate(h.rhs, 1, precond=3, method=1, b_rows=h.n_data)['bytes_per_iter']
        fs.solver.set_data_bias(ids, c)
        fs.solver.set_data_slope(grp, u, cs)
        assert _mode(fs.solver) == _want(nt)
        xg, st = fs.solver.solve(h.rhs, maxit=8, precond=3, **ZERO)
        xe, se = fs.solver.solve(h.rhs, maxit=8, precond=3, use_graph=False, **ZERO)
        assert st['method'] == se['method'] == 1 and st['iters'] == se['iters'] == 8
        np.testing.assert_array_equal(xg, xe)
        for f in ('r1norm', 'arnorm', 'xnorm', 'anorm'):
            assert st[f] == se[f], f

        def restart():
            fs.solver.set_data_slope(grp, u, cs)

        prof = _profiler_runs_real_iterations(fs.solver, h.rhs, h.n_data,
                                              lambda reps: fs.solver.profile_cg(reps=reps, precond=3), restart)
        assert (prof['normal_mode'], prof['data_rows']) == _want(nt)
        _times_are_positive([prof[k] for k in ('cg_data', 'cg_normal', 'cg_update', 'cg_scalars')])
        restart()
        ps = _profiler_runs_real_iterations(fs.solver, h.rhs, h.n_data,
                                            lambda reps: fs.solver.profile_data_slope(reps=reps, precond=3), restart)
        print(ps)
        with_elim = fs.solver.iterate(h.rhs, 1, precond=3, method=1, b_rows=h.n_data)['bytes_per_iter']
        assert sum(prof['bytes'].values()) == with_elim > plain > 0
        _times_are_positive([ms for ms, _ in ps.values()])
        assert prof['bytes']['cg_normal'] >= 32.0 * fs.n_full and (nt < 20 or prof['bytes']['cg_normal'] > 32.0 * fs.n_full)
        # the same handle on its stored rows: the normal kernel's model carries the ATd terms there
        fs.solver.set_data_bias(None, None)
        fs.solver.set_cg_tile_dmf(False)
        stored = fs.solver.profile_cg(reps=1, precond=3)
        assert (stored['normal_mode'], stored['data_rows']) == (_want(nt)[0], 'stored')
        assert stored['bytes']['cg_normal'] > prof['bytes']['cg_normal']
    finally:
        fs.close()


# ---- 4. smooth_fit -----------------------------------------------------------------------------------
def _bias_fit(nt, **extra):
    """The frame of tests/test_gpu_bias.py (sys_bias's points, sensor and cycle biases) on nt epochs: the
    same 0.25 spacing over (nt − 1) / 4 instead of 1.25 (test_gpu_cgnr_tile._bias_16, restated)"""
    from conftest import golden, golden_kwargs, golden_points
    g = golden('sys_bias.npz')
    kw = golden_kwargs(g)
    kw.update(W=dict(kw['W'], t=0.25 * (nt - 1)), reference_epoch=nt // 2, max_iterations=1)
    S = LS.smooth_fit(data=golden_points(g), **kw, **extra)
    assert S['m']['dz'].dz.shape[2] == nt
    return S


@functools.lru_cache(maxsize=None)
def _columns(nt):
    return _bias_fit(nt, lsq_bias='columns')


def _same_fit(Se, Sc):
    from test_gpu_bias import _rel
    assert _rel(Se['m']['z0'].z0, Sc['m']['z0'].z0) < 1e-6
    assert _rel(Se['m']['dz'].dz, Sc['m']['dz'].dz) < 1e-6
    assert _rel(Se['data'].z_est, Sc['data'].z_est) < 1e-6
    ve, vc = np.array(Se['m']['bias']['val']), np.array(Sc['m']['bias']['val'])
    assert np.any(vc != 0) and np.linalg.norm(ve - vc) <= 1e-6 * np.linalg.norm(vc)


@pytest.mark.parametrize('nt', [16, 28])
@pytest.mark.parametrize('mode', ['eliminate', 'auto'])
def test_smooth_fit_eliminates_with_the_key(gpu_available, nt, mode):
    """lsq_bias='eliminate' (and 'auto' above lsq_dense_max) with lsq_tile_eliminate, at 28 epochs beside
    lsq_cg_chunks: CGNR with block-Jacobi, the fit of lsq_bias='columns'"""
    Se = _bias_fit(nt, lsq_bias=mode, lsq_dense_max=0, lsq_tile_eliminate=True, lsq_cg_chunks=nt >= 20)
    last = Se['timing']['lsq_last']
    assert last['method'] == 1 and last['precond'] == 3, last
    assert Se['timing']['tile_eliminate'] is True
    assert Se['timing']['cg_chunks'] is (nt >= 20)
    _same_fit(Se, _columns(nt))
    assert _columns(nt)['timing']['tile_eliminate'] is False


# ---- 5. the key off, or out of its range, changes nothing -------------------------------------------
def test_column_mode_is_bit_identical_with_the_key(gpu_available):
    h = _host(DENSE, 15)
    xs = []
    for on in (False, True):
        fs = _open(h, **_kw(15, on))
        try:
            assert _mode(fs.solver) == ('column', 'matrix-free')
            x, st = fs.solver.solve(h.rhs, maxit=7, precond=3, **ZERO)
            assert st['method'] == 1 and st['iters'] == 7
            xs.append(x)
        finally:
            fs.close()
    np.testing.assert_array_equal(xs[0], xs[1])


def test_without_the_key_tile_mode_still_refuses_biases(gpu_available):
    h = _host(DENSE, 16)
    rng = np.random.default_rng(23)
    ids, c = rng.integers(0, 5, h.n_data).astype(np.int32), rng.uniform(1., 30., 5)
    fs = _open(h)
    try:
        assert _mode(fs.solver) == ('tile', 'stored')
        fs.solver.set_data_bias(ids, c)
        for p in (1, 3):
            ok, why = fs.solver.cg_available(p)
            assert not ok and 'tile mode is not covered' in why, why
    finally:
        fs.close()
    # 17 epochs without the key: no point table, the set call itself refuses, as before
    fs = _open(_host(DENSE, 17))
    try:
        assert _mode(fs.solver) == ('tile', 'stored')
        with pytest.raises(NativeError):
            fs.solver.set_data_bias(ids, c)
    finally:
        fs.close()


def test_a_virtual_rank_refuses_the_key(gpu_available):
    L = load()
    g = L.lsq_vgroup_create(0, 2)
    assert g
    try:
        hr = L.lsq_vgroup_rank(g, 1)
        assert L.lsq_set_cg_tile_dmf(hr, 1) == L.lsq_set_cg_chunks(hr, 1) == -2
        assert 'single-GPU' in L.lsq_last_error(hr).decode()
    finally:
        L.lsq_vgroup_destroy(g)


# ---- 6. what stays refused under the key -------------------------------------------------------------
@pytest.mark.parametrize('nt', [17, 28])
def test_refusals_under_the_key_leave_the_handle_usable(gpu_available, nt):
    h = _host(DENSE, nt)
    rng = np.random.default_rng(61)
    ids, c = rng.integers(0, 5, h.n_data).astype(np.int32), rng.uniform(1., 30., 5)
    fs = _open(h, **_kw(nt))
    try:
        assert _mode(fs.solver) == _want(nt)
        x0, st = fs.solver.solve(h.rhs, precond=3, method=1, **TOL)
        assert st['method'] == 1
        ok, why = fs.solver.cg_available(4)
        assert not ok and 'needs the column-mode normal-stencil operator' in why, why
        assert not fs.multigrid_available()
        x, st = fs.solver.solve(h.rhs, precond=3, method=1, **TOL)
        assert st['method'] == 1 and np.array_equal(x, x0)
        # biases: precond 4 refused with them too, precond 3 runs; cleared, the plain bits return
        fs.solver.set_data_bias(ids, c)
        ok, why = fs.solver.cg_available(4)
        assert not ok and 'column-mode' in why, why
        xb, st = fs.solver.solve(h.rhs, precond=3, method=1, **TOL)
        assert st['method'] == 1 and np.any(xb != x0) and np.any(fs.solver.data_bias() != 0)
        fs.solver.set_data_bias(None, None)
        x, st = fs.solver.solve(h.rhs, precond=3, method=1, **TOL)
        assert np.array_equal(x, x0)
        # the key off again on this handle: the stored rows, and the biases refused as without it
        fs.solver.set_cg_tile_dmf(False)
        assert _mode(fs.solver) == (_want(nt)[0], 'stored')
        fs.solver.set_cg_tile_dmf(True)
        assert _mode(fs.solver) == _want(nt)
    finally:
        fs.close()


def test_extra_rows_still_take_the_coo_path(gpu_available):
    nt = 17
    h = _host(DENSE, nt)
    csr, wx, prior = H.frame_priors(h, h.S['grids']['dz'].shape[2] // 2)
    W, b = np.r_[h.w, wx], np.r_[h.rhs, prior]
    A = sp.vstack([h.A(), H.extra_rows_host(h, csr, wx)]).tocsr()
    xs = ls_solve_dense(A, W * b)
    with pytest.warns(RuntimeWarning, match='extra rows need the column-mode CGNR operator'):
        fs = h.fit_system(extra_csr=csr, **_kw(nt))
    try:
        assert fs.formation == 'coo' and fs.n_extra == 0
        x = fs.solve(W, np.ones(h.n_data, bool), b, maxit=200000, precond=3, method=1, **TOL)
        st = fs.stats
    finally:
        fs.close()
    assert st['method'] == 0 and st['istop'] in (1, 2), st
    rel = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    assert rel <= REL and np.max(np.abs(x - xs)) <= ABS, rel


def test_20_epochs_without_chunks_and_65_epochs_have_no_operator(gpu_available):
    rng = np.random.default_rng(71)
    for shape, npts, nt, chunks, word in ((DENSE, 1200, 20, False, 'LDS'), ((5, 6), 400, 65, True, '64 nodes')):
        h = T.host(shape, npts, nt)
        ids, c = rng.integers(0, 5, h.n_data).astype(np.int32), rng.uniform(1., 30., 5)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            with pytest.raises(NativeError):
                h.fit_system(bias=(ids, c), tile_dmf=True, cg_chunks=chunks)
        fs = h.fit_system(tile_dmf=True, cg_chunks=chunks)
        try:
            ok, why = fs.solver.cg_available(3)
            assert not ok and word in why, why
        finally:
            fs.close()
