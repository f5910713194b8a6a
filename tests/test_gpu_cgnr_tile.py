"""CGNR (lsq method 1) with 16 and more epochs, where the normal operator leaves column mode
(cg_layout in lsqr_cg.inc): smooth_fit's dz stencil reaches 2 nodes along every dimension, a strip
row of 64 + 4 nodes with 16 epochs (padded to 17) no longer fits the ring's 1 024 row-image columns,
and the whole system, z0 grid included, runs tile mode: k_cg_normal on p = z + β p_old staged per
tile, the stored Ad / ATd data rows, the step in the order AD, NORMAL, and the block update
k_cg_block<true, BJ_LANES> (16 epochs: affine blocks of 16) or k_cg_block<false, BJ_LANES> (17 and
more: node_column_blocks splits a node's columns into 16 + rest).  A tile of 20 epochs no longer fits
64 KB of LDS: no CGNR operator, method 1 runs LSQR and says so.

Every case asserts the mode it ran in, so that a change of cg_layout cannot move these cases back to
column mode unnoticed.  The references are those of tests/test_gpu_cgnr_iterates.py (host PCG with
bf16-rounded factors in extended precision, τ_k = max(1000·e_k, 1e-13)) on the host-formed A, and
oracle.dense.ls_solve_dense under DESIGN.md's REL 1e-6 / ABS 1e-4 for the converged solves.  Device
solves run before get_csr(), as that file's header explains.  With CGNR_ITERATES_JSON set the figures
go to that file (profiles/cgnr_iterates_tile.json is one such run of this file alone).

Found by these tests and fixed in FitSystem (lssurf_amd/smooth_fit.py):
  * biases, slopes and sensor grids at exactly 16 epochs: the device accepted lsq_set_data_bias (the
    data rows are matrix-free up to CG_MAXT = 16 nodes) and refused every solve (tile mode does not
    eliminate), so smooth_fit(lsq_bias='auto') raised at its first solve instead of taking 'columns'.
    FitSystem now asks cg_available once the eliminations are set and raises at construction
    (test_smooth_fit_bias_auto_takes_columns_at_16_epochs).
  * extra rows at 16 and more epochs: the formation succeeded and every solve raised ('extra rows need
    the column-mode CGNR operator'); only LSQR with precond 2 or 5 ran.  FitSystem now asks cg_available
    behind the formation, unless its caller solves that way alone (iterative=False), and takes the COO
    path with its warning, for extra_csr too (test_extra_rows_take_the_coo_path)."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import conftest  # noqa: F401
import cgnr_host as H
import lssurf_amd as LS
from lssurf_amd._native import LsqStats, NativeError, as_c, default_opts, ptr
from oracle.dense import ls_solve_dense
from test_gpu_cgnr import ABS, REL, TOL, _profiler_runs_real_iterations, _times_are_positive
from test_gpu_cgnr_iterates import EST, EST_TOL, RECORD, ZERO, Ref, _blocks, _check_iterates, _open, _same_as_host, _solves

pytestmark = pytest.mark.gpu
KS9 = H.KS9
SWEEP = [(shape, nt) for shape, _ in H.TILE_SWEEP for nt in H.TILE_NT]
NPTS = dict(H.TILE_SWEEP + [H.TILE_DENSE])
DENSE = H.TILE_DENSE[0]
BLOCK_SIZES = {15: [15], 16: [16], 17: [1, 16], 19: [3, 16], 20: [4, 16]}


def _host(shape, nt):
    return H.ksweep_host(shape, NPTS[shape], nt)


def _name(shape, nt, tag=''):
    return f'tile-{shape[0]}x{shape[1]}-{nt}' + (f'-{tag}' if tag else '')


# ---- cg_layout's rule, restated --------------------------------------------------------------------
CG_TX, CG_MAXT, CG_NCW, LDS_BYTES, H_DZ = 64, 16, 16, 64 * 1024, 2


def layout_rule(S0, S2, h=H_DZ):
    """The mode of a grid of S0 rows and S2 nodes along dim 2 whose normal stencil reaches h nodes
    along every dimension: 'column', 'tile', or the refusal ('lds', 'nodes')."""
    if S2 > 64:
        return 'nodes'
    tpad = S2 if S2 & 1 else S2 + 1            # LDS stride of a node column: odd
    wx = CG_TX + 2 * h
    if S2 <= CG_MAXT and wx * tpad <= CG_NCW * 64:
        return 'column'
    ty = max(1, min(S0, 48 // S2, 64 // S2))
    return 'tile' if (h + (ty + 2 * h) * wx * tpad + h) * 8 <= LDS_BYTES else 'lds'


def test_layout_rule_restated():
    """The figures the issue quotes: 68·15 = 1 020 columns at 15 epochs, 8 096 doubles at 16."""
    assert [layout_rule(9, nt) for nt in (2, 13, 15, 16, 17, 19, 20, 64, 65)] == \
        ['column', 'column', 'column', 'tile', 'tile', 'tile', 'lds', 'lds', 'nodes']
    assert 68 * 15 == 1020 and 2 + (3 + 4) * 68 * 17 + 2 == 8096 and 8192 * 8 - 8096 * 8 == 768


def _mode(solver, precond=3):
    """(normal_mode, data_rows) of profile_cg; drops the live state, so before the solves"""
    p = solver.profile_cg(reps=1, precond=precond)
    return p['normal_mode'], p['data_rows']


def _open_any(h):
    """a handle with h's weights and every row kept, whatever operator it has"""
    fs = h.fit_system()
    try:
        assert fs.formation == 'stencil' and fs.has_blocks
        fs.solver.set_row_weight(h.w)
        fs.solver.set_row_mask(np.ones(h.w.size, bool))
    except BaseException:
        fs.close()
        raise
    return fs


# ---- 1. mode table ---------------------------------------------------------------------------------
@pytest.mark.parametrize('nt', [15, 16, 17, 19, 20])
def test_mode_table(gpu_available, nt):
    h = _host(DENSE, nt)
    assert [C.shape[1] for C in _blocks(h)] == BLOCK_SIZES[nt]
    want = layout_rule(DENSE[0], nt)
    assert want == {15: 'column', 20: 'lds'}.get(nt, 'tile')
    fs = _open_any(h)
    try:
        got = {p: fs.solver.cg_available(p) for p in (1, 3, 4)}
        print(nt, want, got)
        if want == 'lds':
            for p in (1, 3):
                ok, why = got[p]
                assert not ok and 'LDS' in why, (p, why)
            assert not got[4][0]
        else:
            assert got[1] == (True, '') and got[3] == (True, '')
            assert _mode(fs.solver) == (('column', 'matrix-free') if want == 'column' else ('tile', 'stored'))
            if want == 'tile':
                ok, why = got[4]
                assert not ok and 'needs the column-mode normal-stencil operator' in why, why
    finally:
        fs.close()


# ---- 2. formation and operator, 3. iterates ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _masked(shape, nt):
    """One handle under mask_and_weights: the mode, the iterates of the cases of H.TILE_MASKED, N p on two
    random p, and get_csr() last."""
    h = _host(shape, nt)
    w, mask = H.mask_and_weights(h)
    rng = np.random.default_rng(7)
    ps = [rng.standard_normal(h.keep_cols.size) for _ in range(2)]
    fs = _open(h, w, mask)
    try:
        mode = _mode(fs.solver)
        dev = _solves(fs.solver, h.rhs, KS9) if (shape, nt) in H.TILE_MASKED else None
        qs = []
        for p in ps:
            pf = np.zeros(fs.n_full)
            pf[fs.keep_cols] = p
            qs.append(fs.solver.normal_apply(pf)[fs.keep_cols])
        A = fs.solver.get_csr()
    finally:
        fs.close()
    return h, (w, mask), mode, dev, ps, qs, A


@functools.lru_cache(maxsize=None)
def _plain(shape, nt, precond=3, warm=False):
    """device iterates with h's own weights and every row kept, and their reference"""
    h = _host(shape, nt)
    x0 = H.warm_start(h) if warm else None
    fs = _open(h)
    try:
        mode = _mode(fs.solver, precond)
        dev = _solves(fs.solver, h.rhs, KS9, precond=precond, x0=x0)
    finally:
        fs.close()
    A = h.A()
    factors = H.block_factors(A, _blocks(h)) if precond == 3 else H.jacobi_factors(A)
    return mode, dev, Ref(A, h.w * h.rhs, factors, 9, x0=x0)


@pytest.mark.parametrize('shape, nt', SWEEP)
def test_formation_and_operator_under_mask_and_weights(gpu_available, shape, nt):
    """get_csr() is the host-formed A, and k_cg_normal with the stored ATd is its AᵀA, under a data-row
    mask and re-weighted data rows; (5, 200) has x tiles clear of both edges (xuni)."""
    h, (w, mask), mode, _, ps, qs, A = _masked(shape, nt)
    assert mode == ('tile', 'stored')
    assert [C.shape[1] for C in _blocks(h)] == BLOCK_SIZES[nt]
    Ah = h.A(w, mask)
    _same_as_host(A, Ah)
    for p, q in zip(ps, qs):
        qr = Ah.T @ (Ah @ p)
        err = np.abs(q - qr).max() / np.abs(qr).max()
        print(f'{_name(shape, nt)}: operator {err:.2e}')
        rec = RECORD.setdefault(_name(shape, nt), {})
        rec['operator'] = max(rec.get('operator', 0.0), float(err))   # max|q − AᵀA p| / max|AᵀA p| over the two p
        assert err <= 1e-12, err


@pytest.mark.parametrize('shape, nt', SWEEP)
def test_tile_iterates_match_host_reference(gpu_available, shape, nt):
    """precond 3 on every tile case: affine blocks of 16, and 16 + 1 and 16 + 3 split blocks"""
    mode, dev, ref = _plain(shape, nt)
    assert mode == ('tile', 'stored') and sorted(dev) == list(KS9)
    _check_iterates(_name(shape, nt), dev, ref)


@pytest.mark.parametrize('shape, nt', H.TILE_MASKED)
def test_tile_iterates_under_mask_and_weights(gpu_available, shape, nt):
    h, (w, mask), mode, dev, _, _, _ = _masked(shape, nt)
    assert mode == ('tile', 'stored')
    A = h.A(w, mask)
    _check_iterates(_name(shape, nt, 'mask'), dev, Ref(A, (w * h.rhs)[mask], H.block_factors(A, _blocks(h)), 9))


def test_tile_iterates_jacobi(gpu_available):
    mode, dev, ref = _plain((7, 70), 17, precond=1)
    assert mode == ('tile', 'stored')
    _check_iterates(_name((7, 70), 17, 'jacobi'), dev, ref)


def test_tile_iterates_warm_start(gpu_available):
    mode, dev, ref = _plain((5, 200), 16, warm=True)
    assert mode == ('tile', 'stored')
    _check_iterates(_name((5, 200), 16, 'x0'), dev, ref)


def test_sensitivity_block_normals_that_ignore_the_mask(gpu_available):
    """A reference whose factors come from every row although the operator is masked: more than
    1e3·τ_k from the device, from the first k at which the two references differ by that much."""
    shape, nt = H.TILE_MASKED[0]
    h, (w, mask), _, dev, _, _, _ = _masked(shape, nt)
    A = h.A(w, mask)
    ref = Ref(A, (w * h.rhs)[mask], H.block_factors(A, _blocks(h)), 9)
    xb = H.pcg(A, ref.b, H.block_factors(h.A(w), _blocks(h)), 9, dtype=np.longdouble)['x']
    apart = {k: ref.dev(k, xb[k]) for k in KS9}
    print('masked against unmasked factors:', {k: f'{v:.2e}' for k, v in apart.items()})
    first = min(k for k in KS9 if apart[k] > 1e3 * ref.tau[k])
    assert first <= 2
    for k in KS9:
        if k >= first:
            d = ref.dev(k, dev[k][0], xb[k])
            assert d > 1e3 * ref.tau[k], (k, d, ref.tau[k])


# ---- 4. step mechanics -----------------------------------------------------------------------------
MECH = (7, 70)


@pytest.mark.parametrize('nt', [16, 17])
def test_graph_replay_and_batch_size_leave_the_iterate(gpu_available, nt):
    """use_graph False at k = 2, 5, 8 and batch 4 / 8 / 16 at k = 7: the same x bit for bit"""
    _, dev, _ = _plain(MECH, nt)
    h = _host(MECH, nt)
    fs = _open(h)
    try:
        assert _mode(fs.solver) == ('tile', 'stored')
        eager = _solves(fs.solver, h.rhs, (2, 5, 8), use_graph=False)
        for k in (2, 5, 8):
            np.testing.assert_array_equal(eager[k][0], dev[k][0])
            for f in EST:
                assert eager[k][1][f] == dev[k][1][f], (k, f)
        for batch in (4, 8, 16):
            x, st = fs.solver.solve(h.rhs, maxit=7, precond=3, batch=batch, **ZERO)
            assert st['method'] == 1 and st['istop'] == 7 and st['iters'] == 7
            np.testing.assert_array_equal(x, dev[7][0])
    finally:
        fs.close()


@pytest.mark.parametrize('nt', [16, 17])
def test_iterate_calls_continue_one_run(gpu_available, nt):
    """iterate(5) then iterate(4) stand at the reference's step 9.  r1norm comes from the recurrence
    rn2 −= αρ, which loses ε·k·(‖r0‖/‖r_k‖)²: EST_TOL where that loss, from the reference, stays two
    orders below it, else 100× the loss."""
    _, _, ref = _plain(MECH, nt)
    h = _host(MECH, nt)
    fs = _open(h)
    try:
        assert _mode(fs.solver) == ('tile', 'stored')
        fs.solver.iterate(h.rhs, 5, precond=3, method=1)
        st = fs.solver.iterate(h.rhs, 4, precond=3, method=1)
    finally:
        fs.close()
    want = ref.stats(9)
    loss = np.finfo(float).eps * 9 * (np.linalg.norm(ref.b) / want['r1norm']) ** 2
    tol = EST_TOL if loss <= 1e-2 * EST_TOL else 100 * loss
    print(f'nt={nt}: loss of the reference {loss:.2e}, tolerance {tol:.2e}')
    assert st['iters'] == 9 and st['method'] == 1
    for f in ('r1norm', 'arnorm'):
        err = abs(st[f] - want[f]) / want[f]
        print(f'iterate to 9 {f}: rel {err:.2e}')
        assert err <= tol, (f, st[f], want[f])


@pytest.mark.parametrize('precond', [1, 3])
@pytest.mark.parametrize('nt', [16, 17])
def test_profile_cg_runs_real_iterations_in_tile_mode(gpu_available, nt, precond):
    """The profiler's live path in tile mode's own order (AD, NORMAL): DESIGN.md §CGNR records that it
    once ran column mode's order there, with a stale t and ATd·t applied twice."""
    h = _host(MECH, nt)
    keep = np.random.default_rng(41).random(h.n_data) > 0.1
    fs = _open(h, mask=np.concatenate([keep, np.ones(h.w.size - h.n_data, bool)]))
    try:
        prof = _profiler_runs_real_iterations(
            fs.solver, h.rhs, h.n_data, lambda reps: fs.solver.profile_cg(reps=reps, precond=precond),
            lambda: fs.solver.normal_apply(np.zeros(fs.n_full)), precond=precond)
        assert (prof['normal_mode'], prof['data_rows']) == ('tile', 'stored')
        _times_are_positive([prof[k] for k in ('cg_data', 'cg_normal', 'cg_update', 'cg_scalars')])
        st = fs.solver.iterate(h.rhs, 1, precond=precond, method=1, b_rows=h.n_data)
        assert sum(prof['bytes'].values()) == st['bytes_per_iter'] > 0
    finally:
        fs.close()


# ---- 5. converged solves, 6. the fallback ------------------------------------------------------------
def _close_to(x, xs):
    rel = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print(f'rel {rel:.2e}, abs {np.max(np.abs(x - xs)):.2e}')
    assert rel <= REL and np.max(np.abs(x - xs)) <= ABS


@functools.lru_cache(maxsize=None)
def _exact(shape, nt):
    h = _host(shape, nt)
    return ls_solve_dense(h.A(), h.w * h.rhs)


@pytest.mark.parametrize('nt', [16, 19])
def test_converged_solves_reach_the_dense_oracle(gpu_available, nt):
    h, xs = _host(DENSE, nt), _exact(DENSE, nt)
    fs = _open(h)
    try:
        assert _mode(fs.solver) == ('tile', 'stored')
        for method, precond in ((1, 1), (1, 3), (0, 3)):
            x, st = fs.solver.solve(h.rhs, maxit=200000, precond=precond, method=method, **TOL)
            print(nt, method, precond, st['iters'])
            assert st['method'] == method and st['istop'] in (1, 2), st
            _close_to(x, xs)
    finally:
        fs.close()


def test_20_epochs_fall_back_to_lsqr(gpu_available):
    """no CGNR operator: method 1 runs LSQR with block-Jacobi on the 16 + 4 blocks and says so"""
    h, xs = _host(DENSE, 20), _exact(DENSE, 20)
    fs = _open_any(h)
    try:
        assert not fs.solver.cg_available(3)[0]
        x, st = fs.solver.solve(h.rhs, maxit=200000, precond=3, method=1, **TOL)
    finally:
        fs.close()
    assert st['method'] == 0 and st['istop'] in (1, 2), st
    _close_to(x, xs)


def test_65_epochs_are_refused_and_solve_through_lsqr(gpu_available):
    shape, npts, nt = (5, 6), 400, 65
    assert layout_rule(shape[0], nt) == 'nodes'
    h = H.ksweep_host(shape, npts, nt)
    xs = ls_solve_dense(h.A(), h.w * h.rhs)
    fs = _open_any(h)
    try:
        for p in (1, 3):
            ok, why = fs.solver.cg_available(p)
            assert not ok and '64 nodes' in why and 'LDS' not in why, why
        x, st = fs.solver.solve(h.rhs, maxit=200000, precond=3, method=1, **TOL)
    finally:
        fs.close()
    assert st['method'] == 0 and st['istop'] in (1, 2), st
    _close_to(x, xs)


# ---- 7. refusals that must stay clean in tile mode (16 epochs) ---------------------------------------
def test_biases_are_refused_at_solve_and_never_dropped(gpu_available):
    """lsq_set_data_bias accepts 16 epochs (matrix-free data rows), tile mode cannot eliminate: every
    solve must raise, never run without the elimination; the handle stays usable."""
    h = _host(DENSE, 16)
    rng = np.random.default_rng(23)
    ids, c = rng.integers(0, 5, h.n_data).astype(np.int32), rng.uniform(1., 30., 5)
    fs = _open(h)
    try:
        x_plain, _ = fs.solver.solve(h.rhs, precond=3, method=1, **TOL)
        fs.solver.set_data_bias(ids, c)
        for p in (1, 3):
            ok, why = fs.solver.cg_available(p)
            assert not ok and 'tile mode is not covered' in why, why
        for method, precond in ((1, 3), (1, 1), (0, 3)):
            with pytest.raises(NativeError):
                fs.solver.solve(h.rhs, precond=precond, method=method, **TOL)
            with pytest.raises(NativeError):
                fs.solver.iterate(h.rhs, 2, precond=precond, method=method)
            # LSQSolver.solve owns x and drops it when it raises: lsq_solve itself on a caller's x
            x_in = rng.standard_normal(h.keep_cols.size)
            x, b, st = x_in.copy(), as_c(h.rhs, np.float64), LsqStats()
            o = default_opts(precond=precond, method=method, use_x0=1, **TOL)
            rc = fs.solver._L.lsq_solve(fs.solver._h, ptr(b), ptr(x), ctypes.byref(o), ctypes.byref(st))
            assert rc < 0 and np.array_equal(x, x_in), (method, precond, rc)
        fs.solver.set_data_bias(None, None)
        x, st = fs.solver.solve(h.rhs, precond=3, method=1, **TOL)
        assert st['method'] == 1 and np.array_equal(x, x_plain)
    finally:
        fs.close()
    with pytest.raises(NativeError, match='tile mode is not covered'):   # FitSystem asks at construction
        h.fit_system(bias=(ids, c))


def test_extra_rows_take_the_coo_path(gpu_available):
    """Extra rows need column mode: FitSystem warns, forms everything from triplets (extra_csr's rows
    behind Gc's) and solves [A; X] through LSQR."""
    h = _host(DENSE, 16)
    csr, wx, prior = H.frame_priors(h, h.S['grids']['dz'].shape[2] // 2)
    W, b = np.r_[h.w, wx], np.r_[h.rhs, prior]
    A = sp.vstack([h.A(), H.extra_rows_host(h, csr, wx)]).tocsr()
    xs = ls_solve_dense(A, W * b)
    with pytest.warns(RuntimeWarning, match='extra rows need the column-mode CGNR operator'):
        fs = h.fit_system(extra_csr=csr)
    try:
        assert fs.formation == 'coo' and fs.n_extra == 0 and fs.n_con == h.w.size - h.n_data + wx.size
        x = fs.solve(W, np.ones(h.n_data, bool), b, maxit=200000, precond=3, method=1, **TOL)
        st = fs.stats
        _same_as_host(fs.solver.get_csr(), A)
    finally:
        fs.close()
    assert st['method'] == 0 and st['istop'] in (1, 2), st
    _close_to(x, xs)
    assert np.linalg.norm(xs - _exact(DENSE, 16)) > 1e-3 * np.linalg.norm(xs)   # the rows do act
    # a caller that solves with the dense preconditioner alone keeps the stencil-formed system
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        fs = h.fit_system(extra_csr=csr, iterative=False)
    try:
        assert fs.formation == 'stencil' and fs.n_extra == wx.size
        x = fs.solve(W, np.ones(h.n_data, bool), b, precond=2, method=0, **TOL)
        assert fs.stats['method'] == 0 and fs.stats['istop'] in (1, 2), fs.stats
    finally:
        fs.close()
    _close_to(x, xs)


@pytest.mark.parametrize('nt, method', [(16, 1), (20, 0)])
def test_smooth_fit_end_to_end(gpu_available, nt, method):
    """One solve of smooth_fit with the iterative path forced: the dense oracle's x on the grids, CGNR in
    tile mode at 16 epochs and LSQR at 20, and the count / misfit maps finite where the host sums are
    (at 17 and more epochs the device's node gather is unavailable: parse_model's host path)."""
    h, xs = _host(DENSE, nt), _exact(DENSE, nt)
    D, kw = H.ksweep_points(DENSE, NPTS[DENSE], nt)
    out = LS.smooth_fit(data=D, max_iterations=1, lsq_dense_max=0, VERBOSE=False, **kw)
    last = out['timing']['lsq_last']
    assert last['method'] == method and last['precond'] == 3, last
    m0 = np.zeros(h.n_full)
    m0[h.keep_cols] = xs
    G = h.S['G_data']
    tse = np.asarray(out['data'].three_sigma_edit, bool).ravel()
    assert tse.size == h.n_data
    count = np.asarray(abs(G.toCSR()[np.flatnonzero(tse)]).sum(axis=0)).ravel()
    for ff, got in (('z0', out['m']['z0'].z0), ('dz', out['m']['dz'].dz)):
        cols = G.TOC['cols'][ff]
        want = m0[cols].reshape(got.shape)
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        print(f'nt={nt} {ff}: rel {rel:.2e}')
        assert rel <= 1e-6
        seen = (count[cols] != 0).reshape(got.shape)
        assert seen.any()
        for name in ('count', 'misfit_rms', 'misfit_scaled_rms'):
            assert np.array_equal(np.isfinite(getattr(out['m'][ff], name)), seen), (ff, name)


def _bias_16(**extra):
    """The frame of tests/test_gpu_bias.py (sys_bias's points, sensor and cycle biases) on 16 epochs: the
    same 0.25 spacing over 3.75 instead of 1.25"""
    from conftest import golden, golden_kwargs, golden_points
    g = golden('sys_bias.npz')
    kw = golden_kwargs(g)
    kw.update(W=dict(kw['W'], t=3.75), reference_epoch=8, max_iterations=1)
    S = LS.smooth_fit(data=golden_points(g), **kw, **extra)
    assert S['m']['dz'].dz.shape[2] == 16
    return S


def test_smooth_fit_bias_auto_takes_columns_at_16_epochs(gpu_available):
    """lsq_bias='auto' above lsq_dense_max at 16 epochs: the README's promise is 'columns' where the
    device cannot eliminate.  It raised at the first solve before FitSystem asked cg_available at
    construction; 'eliminate' raises there, not in the middle of the fit."""
    from test_gpu_bias import _rel
    Sc = _bias_16(lsq_bias='columns')
    Sa = _bias_16(lsq_bias='auto', lsq_dense_max=0)
    assert Sa['timing']['lsq_last']['method'] == 0, Sa['timing']['lsq_last']
    assert _rel(Sa['m']['z0'].z0, Sc['m']['z0'].z0) < 1e-6
    assert _rel(Sa['m']['dz'].dz, Sc['m']['dz'].dz) < 1e-6
    assert _rel(Sa['data'].z_est, Sc['data'].z_est) < 1e-6
    va, vc = np.array(Sa['m']['bias']['val']), np.array(Sc['m']['bias']['val'])
    assert np.any(vc != 0) and np.linalg.norm(va - vc) <= 1e-6 * np.linalg.norm(vc)
    with pytest.raises(NativeError, match='tile mode is not covered'):
        _bias_16(lsq_bias='eliminate', lsq_dense_max=0)
