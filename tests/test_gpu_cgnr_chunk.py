"""CGNR (lsq method 1) with 20 to 64 epochs: chunk mode (lsq_set_cg_chunks, FitSystem(cg_chunks=True),
smooth_fit(lsq_cg_chunks=True)).  A tile of whole time columns no longer fits 64 KB of LDS there; with the
key the normal operator's tiles are also cut along dim 2 (k_cg_normal_chunk: a workgroup per (tile,
chunk), each chunk staged with a halo of 2 nodes along dim 2 as well), and everything else is tile mode's:
the stored Ad / ATd data rows, the step in the order AD, NORMAL, and k_cg_block<false, BJ_LANES> on node
blocks of 16 + 16 + … columns.  Without the key method 1 runs LSQR, as before.

Every case asserts the mode it ran in.  The layout rule is restated in tests/test_cgnr_chunk_host.py,
which also holds the inputs of these cases to test_cgnr_host.py's rounding-boundary condition.  The
references are those of tests/test_gpu_cgnr_tile.py: host PCG with bf16-rounded factors in extended
precision (τ_k = max(1000·e_k, 1e-13)) on the host-formed A, AᵀA p within 1e-12 of max |AᵀA p|, and
oracle.dense.ls_solve_dense under DESIGN.md's REL 1e-6 / ABS 1e-4 for the converged solves.  Device
solves run before get_csr(), as tests/test_gpu_cgnr_iterates.py explains.  With CGNR_ITERATES_JSON set the
figures go to that file (profiles/cgnr_iterates_chunk.json is one such run of this file alone).

Cases: (7, 70) has two x tiles that both touch an edge, the right one 6 columns wide, and rows that are no
multiple of ty; (5, 200) has x tiles clear of both edges (xuni).  20 epochs give unequal chunks (6 + 7 + 7);
41 and 64 give interior chunks with a halo on both sides, and node blocks of 16 + 16 + 9 and 4 × 16."""
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import conftest  # noqa: F401
import cgnr_host as H
import lssurf_amd as LS
from lssurf_amd._native import NativeError, load
from oracle.dense import ls_solve_dense
from test_cgnr_chunk_host import (CHUNK_DENSE, CHUNK_DENSE_NT, CHUNK_MASKED, CHUNK_SWEEP, H_DZ, _lds, chunk_rule,
                                  mode_rule)
from test_gpu_cgnr import ABS, REL, TOL, _profiler_runs_real_iterations, _times_are_positive
from test_gpu_cgnr_iterates import EST_TOL, RECORD, ZERO, Ref, _blocks, _check_iterates, _open, _same_as_host, _solves

pytestmark = pytest.mark.gpu
KS9 = H.KS9
NPTS = {(7, 70): 600, (5, 200): 900, (9, 11): 300}
CHUNK = ('chunk', 'stored')


def _host(shape, nt):
    return H.ksweep_host(shape, NPTS[shape], nt)


def _name(shape, nt, tag=''):
    return f'chunk-{shape[0]}x{shape[1]}-{nt}' + (f'-{tag}' if tag else '')


def _mode(solver, precond=3):
    """(normal_mode, data_rows) of profile_cg; drops the live state, so before the solves"""
    p = solver.profile_cg(reps=1, precond=precond)
    return p['normal_mode'], p['data_rows']


def _open_any(h, chunks):
    """a handle with h's weights and every row kept, whatever operator it has"""
    fs = h.fit_system(cg_chunks=chunks)
    try:
        assert fs.formation == 'stencil' and fs.has_blocks
        fs.solver.set_row_weight(h.w)
        fs.solver.set_row_mask(np.ones(h.w.size, bool))
    except BaseException:
        fs.close()
        raise
    return fs


# ---- 1. mode table ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seven_steps(nt, chunks):
    """(layout info, profile_cg's mode or None, x after 7 iterations or None) on (9, 11)"""
    h = _host(CHUNK_DENSE, nt)
    fs = _open_any(h, chunks)
    try:
        info = fs.solver.cg_layout_info()
        if info['mode'] == 'none':
            return info, None, None
        mode = _mode(fs.solver)
        x, st = fs.solver.solve(h.rhs, maxit=7, precond=3, **ZERO)
        assert st['method'] == 1 and st['iters'] == 7
        return info, mode, x
    finally:
        fs.close()


@pytest.mark.parametrize('nt', [15, 16, 19, 20, 28, 64])
def test_mode_table(gpu_available, nt):
    S0 = CHUNK_DENSE[0]
    want = mode_rule(S0, nt, True)
    assert want == {15: 'column', 16: 'tile', 19: 'tile'}.get(nt, 'chunk')
    on, mode_on, x_on = _seven_steps(nt, True)
    off, mode_off, x_off = _seven_steps(nt, False)
    print(nt, on, off)
    assert on['mode'] == want and mode_on == (want, 'matrix-free' if want == 'column' else 'stored')
    if want == 'chunk':
        ty, tc, nch, tcpad = chunk_rule(S0, nt)
        assert (on['ty'], on['tc'], on['chunks'], on['tcpad']) == (ty, tc, nch, tcpad)
        assert on['lds_bytes'] == _lds(ty, tc, H_DZ) * 8 <= 64 * 1024
        # the z0 grid keeps its tile-mode geometry as one chunk: one tile of 9 rows; then the dz grid's
        tiles = 1 + -(-S0 // ty) * nch
        assert on['workgroups'] == 8 * -(-tiles // 8)
        # without the key: today's refusal
        assert off['mode'] == 'none' and 'LDS' in off['reason'] and mode_off is None
    else:
        # the key changes nothing where column or tile mode runs: the same layout, the same x bit for bit
        assert off == on and mode_off == mode_on
        np.testing.assert_array_equal(x_on, x_off)


# ---- 2. formation and operator, 3. iterates ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _masked(shape, nt):
    """One handle under mask_and_weights: the mode, the iterates of the cases of CHUNK_MASKED, N p on two
    random p, and get_csr() last."""
    h = _host(shape, nt)
    w, mask = H.mask_and_weights(h)
    rng = np.random.default_rng(7)
    ps = [rng.standard_normal(h.keep_cols.size) for _ in range(2)]
    fs = _open(h, w, mask, cg_chunks=True)
    try:
        mode = _mode(fs.solver)
        dev = _solves(fs.solver, h.rhs, KS9) if (shape, nt) in CHUNK_MASKED else None
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
    fs = _open(h, cg_chunks=True)
    try:
        mode = _mode(fs.solver, precond)
        dev = _solves(fs.solver, h.rhs, KS9, precond=precond, x0=x0)
    finally:
        fs.close()
    A = h.A()
    factors = H.block_factors(A, _blocks(h)) if precond == 3 else H.jacobi_factors(A)
    return mode, dev, Ref(A, h.w * h.rhs, factors, 9, x0=x0)


@pytest.mark.parametrize('shape, nt', CHUNK_SWEEP)
def test_formation_and_operator_under_mask_and_weights(gpu_available, shape, nt):
    """get_csr() is the host-formed A, and k_cg_normal_chunk with the stored ATd is its AᵀA, under a
    data-row mask and re-weighted data rows.  The bound is the tile tests' (7.0e-16 … 9.7e-16 measured
    there)."""
    h, (w, mask), mode, _, ps, qs, A = _masked(shape, nt)
    assert mode == CHUNK
    assert sorted({C.shape[1] for C in _blocks(h)}) == sorted({16, nt % 16} - {0})
    Ah = h.A(w, mask)
    _same_as_host(A, Ah)
    for p, q in zip(ps, qs):
        qr = Ah.T @ (Ah @ p)
        err = np.abs(q - qr).max() / np.abs(qr).max()
        print(f'{_name(shape, nt)}: operator {err:.2e}')
        rec = RECORD.setdefault(_name(shape, nt), {})
        rec['operator'] = max(rec.get('operator', 0.0), float(err))   # max|q − AᵀA p| / max|AᵀA p| over the two p
        assert err <= 1e-12, err


@pytest.mark.parametrize('shape, nt', CHUNK_SWEEP)
def test_chunk_iterates_match_host_reference(gpu_available, shape, nt):
    """precond 3 on every chunk case"""
    mode, dev, ref = _plain(shape, nt)
    assert mode == CHUNK and sorted(dev) == list(KS9)
    _check_iterates(_name(shape, nt), dev, ref)


@pytest.mark.parametrize('shape, nt', CHUNK_MASKED)
def test_chunk_iterates_under_mask_and_weights(gpu_available, shape, nt):
    h, (w, mask), mode, dev, _, _, _ = _masked(shape, nt)
    assert mode == CHUNK
    A = h.A(w, mask)
    _check_iterates(_name(shape, nt, 'mask'), dev, Ref(A, (w * h.rhs)[mask], H.block_factors(A, _blocks(h)), 9))


def test_chunk_iterates_jacobi(gpu_available):
    mode, dev, ref = _plain((7, 70), 28, precond=1)
    assert mode == CHUNK
    _check_iterates(_name((7, 70), 28, 'jacobi'), dev, ref)


def test_chunk_iterates_warm_start(gpu_available):
    mode, dev, ref = _plain((5, 200), 20, warm=True)
    assert mode == CHUNK
    _check_iterates(_name((5, 200), 20, 'x0'), dev, ref)


# ---- 4. step mechanics -----------------------------------------------------------------------------
MECH = (7, 70)


@pytest.mark.parametrize('nt', [20, 41])
def test_graph_replay_and_batch_size_leave_the_iterate(gpu_available, nt):
    """use_graph False at k = 2, 5, 8 and batch 4 / 8 / 16 at k = 7: the same x bit for bit"""
    _, dev, _ = _plain(MECH, nt)
    h = _host(MECH, nt)
    fs = _open(h, cg_chunks=True)
    try:
        assert _mode(fs.solver) == CHUNK
        eager = _solves(fs.solver, h.rhs, (2, 5, 8), use_graph=False)
        for k in (2, 5, 8):
            np.testing.assert_array_equal(eager[k][0], dev[k][0])
            for f in ('r1norm', 'arnorm', 'xnorm', 'anorm'):
                assert eager[k][1][f] == dev[k][1][f], (k, f)
        for batch in (4, 8, 16):
            x, st = fs.solver.solve(h.rhs, maxit=7, precond=3, batch=batch, **ZERO)
            assert st['method'] == 1 and st['istop'] == 7 and st['iters'] == 7
            np.testing.assert_array_equal(x, dev[7][0])
    finally:
        fs.close()


@pytest.mark.parametrize('nt', [20, 41])
def test_iterate_calls_continue_one_run(gpu_available, nt):
    """iterate(5) then iterate(4) stand at the reference's step 9, under the tolerance rule of
    tests/test_gpu_cgnr_tile.py: r1norm comes from the recurrence rn2 −= αρ, which loses
    ε·k·(‖r0‖/‖r_k‖)²; EST_TOL where that loss, from the reference, stays two orders below it, else
    100× the loss."""
    _, _, ref = _plain(MECH, nt)
    h = _host(MECH, nt)
    fs = _open(h, cg_chunks=True)
    try:
        assert _mode(fs.solver) == CHUNK
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
@pytest.mark.parametrize('nt', [20, 41])
def test_profile_cg_runs_real_iterations_in_chunk_mode(gpu_available, nt, precond):
    """The profiler's live path in tile mode's order (AD, NORMAL), and the byte model of chunk mode:
    the total of profile_cg is what iterate() reports."""
    h = _host(MECH, nt)
    keep = np.random.default_rng(41).random(h.n_data) > 0.1
    fs = _open(h, mask=np.concatenate([keep, np.ones(h.w.size - h.n_data, bool)]), cg_chunks=True)
    try:
        prof = _profiler_runs_real_iterations(
            fs.solver, h.rhs, h.n_data, lambda reps: fs.solver.profile_cg(reps=reps, precond=precond),
            lambda: fs.solver.normal_apply(np.zeros(fs.n_full)), precond=precond)
        assert (prof['normal_mode'], prof['data_rows']) == CHUNK
        _times_are_positive([prof[k] for k in ('cg_data', 'cg_normal', 'cg_update', 'cg_scalars')])
        st = fs.solver.iterate(h.rhs, 1, precond=precond, method=1, b_rows=h.n_data)
        assert sum(prof['bytes'].values()) == st['bytes_per_iter'] > 0
        # z and p_old over the staged images, p and q over the owned entries: more than tile mode's 32 B
        # per column, by the halos
        assert prof['bytes']['cg_normal'] > 32.0 * fs.n_full
    finally:
        fs.close()


# ---- 5. converged solves ---------------------------------------------------------------------------
def _close_to(x, xs):
    rel = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print(f'rel {rel:.2e}, abs {np.max(np.abs(x - xs)):.2e}')
    assert rel <= REL and np.max(np.abs(x - xs)) <= ABS


@functools.lru_cache(maxsize=None)
def _exact(shape, nt):
    h = _host(shape, nt)
    return ls_solve_dense(h.A(), h.w * h.rhs)


@pytest.mark.parametrize('nt', CHUNK_DENSE_NT)
def test_converged_solves_reach_the_dense_oracle(gpu_available, nt):
    """method 1 runs CGNR with the key and LSQR without it; both reach the dense oracle"""
    h, xs = _host(CHUNK_DENSE, nt), _exact(CHUNK_DENSE, nt)
    for chunks, method in ((True, 1), (False, 0)):
        fs = _open_any(h, chunks)
        try:
            if chunks:
                assert _mode(fs.solver) == CHUNK
            for precond in (1, 3):
                x, st = fs.solver.solve(h.rhs, maxit=200000, precond=precond, method=1, **TOL)
                print(nt, chunks, precond, st['method'], st['iters'])
                assert st['method'] == method and st['istop'] in (1, 2), st
                _close_to(x, xs)
        finally:
            fs.close()


# ---- 6. what stays refused with the key on ---------------------------------------------------------
def test_65_epochs_are_refused_and_solve_through_lsqr(gpu_available):
    shape, npts, nt = (5, 6), 400, 65
    assert mode_rule(shape[0], nt, True) == 'nodes'
    h = H.ksweep_host(shape, npts, nt)
    xs = ls_solve_dense(h.A(), h.w * h.rhs)
    fs = _open_any(h, True)
    try:
        info = fs.solver.cg_layout_info()
        assert info['mode'] == 'none' and '64 nodes' in info['reason'], info
        for p in (1, 3):
            ok, why = fs.solver.cg_available(p)
            assert not ok and '64 nodes' in why and 'LDS' not in why, why
        x, st = fs.solver.solve(h.rhs, maxit=200000, precond=3, method=1, **TOL)
    finally:
        fs.close()
    assert st['method'] == 0 and st['istop'] in (1, 2), st
    _close_to(x, xs)


def test_multigrid_is_refused_in_chunk_mode(gpu_available):
    fs = _open_any(_host(CHUNK_DENSE, 20), True)
    try:
        assert fs.solver.cg_available(3) == (True, '') and _mode(fs.solver) == CHUNK
        ok, why = fs.solver.cg_available(4)
        assert not ok and 'needs the column-mode normal-stencil operator' in why, why
        assert not fs.multigrid_available()
        # switching the key off and on again lays out afresh
        fs.solver.set_cg_chunks(False)
        ok, why = fs.solver.cg_available(3)
        assert not ok and 'LDS' in why, why
        fs.solver.set_cg_chunks(True)
        assert fs.solver.cg_available(3) == (True, '') and fs.solver.cg_layout_info()['mode'] == 'chunk'
    finally:
        fs.close()


def test_biases_raise_at_construction(gpu_available):
    h = _host(CHUNK_DENSE, 20)
    rng = np.random.default_rng(23)
    ids, c = rng.integers(0, 5, h.n_data).astype(np.int32), rng.uniform(1., 30., 5)
    with pytest.raises(NativeError):
        h.fit_system(bias=(ids, c), cg_chunks=True)


def test_extra_rows_take_the_coo_path(gpu_available):
    """Extra rows need column mode: FitSystem warns, forms everything from triplets and solves [A; X]
    through LSQR, as at 16 epochs."""
    h = _host(CHUNK_DENSE, 20)
    csr, wx, prior = H.frame_priors(h, h.S['grids']['dz'].shape[2] // 2)
    W, b = np.r_[h.w, wx], np.r_[h.rhs, prior]
    A = sp.vstack([h.A(), H.extra_rows_host(h, csr, wx)]).tocsr()
    xs = ls_solve_dense(A, W * b)
    with pytest.warns(RuntimeWarning, match='extra rows need the column-mode CGNR operator'):
        fs = h.fit_system(extra_csr=csr, cg_chunks=True)
    try:
        assert fs.formation == 'coo' and fs.n_extra == 0 and fs.n_con == h.w.size - h.n_data + wx.size
        x = fs.solve(W, np.ones(h.n_data, bool), b, maxit=200000, precond=3, method=1, **TOL)
        st = fs.stats
    finally:
        fs.close()
    assert st['method'] == 0 and st['istop'] in (1, 2), st
    _close_to(x, xs)


def test_a_virtual_rank_refuses_the_key(gpu_available):
    L = load()
    g = L.lsq_vgroup_create(0, 2)
    assert g
    try:
        hr = L.lsq_vgroup_rank(g, 1)
        assert L.lsq_set_cg_chunks(hr, 1) == -2
        assert 'single-GPU' in L.lsq_last_error(hr).decode()
    finally:
        L.lsq_vgroup_destroy(g)


# ---- 7. smooth_fit -----------------------------------------------------------------------------------
def _fit(**extra):
    D, kw = H.ksweep_points(CHUNK_DENSE, NPTS[CHUNK_DENSE], 28)
    return LS.smooth_fit(data=D, max_iterations=1, lsq_precond=3, VERBOSE=False, **kw, **extra)


def test_smooth_fit_key(gpu_available):
    on, off = _fit(lsq_cg_chunks=True), _fit()
    assert on['timing']['cg_chunks'] is True and on['timing']['lsq_last']['method'] == 1
    assert off['timing']['cg_chunks'] is False and off['timing']['lsq_last']['method'] == 0
    for got, want in ((on['m']['z0'].z0, off['m']['z0'].z0), (on['m']['dz'].dz, off['m']['dz'].dz)):
        assert got.shape == want.shape
        _close_to(got.ravel(), want.ravel())
    with pytest.raises(ValueError, match='lsq_cg_chunks'):
        _fit(lsq_cg_chunks=1)


def _bias_28(**extra):
    """The frame of tests/test_gpu_bias.py (sys_bias's points, sensor and cycle biases) on 28 epochs: the
    same 0.25 spacing over 6.75 instead of 1.25"""
    from conftest import golden, golden_kwargs, golden_points
    g = golden('sys_bias.npz')
    kw = golden_kwargs(g)
    kw.update(W=dict(kw['W'], t=6.75), reference_epoch=14, max_iterations=1)
    S = LS.smooth_fit(data=golden_points(g), **kw, **extra)
    assert S['m']['dz'].dz.shape[2] == 28
    return S


def test_smooth_fit_bias_auto_takes_columns(gpu_available):
    """chunk mode does not eliminate: lsq_bias='auto' takes 'columns' with the key, 'eliminate' raises"""
    from test_gpu_bias import _rel
    Sc = _bias_28(lsq_bias='columns')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        Sa = _bias_28(lsq_bias='auto', lsq_dense_max=0, lsq_cg_chunks=True)
    assert Sa['timing']['lsq_last']['method'] == 0 and Sa['timing']['cg_chunks'] is False, Sa['timing']['lsq_last']
    assert _rel(Sa['m']['z0'].z0, Sc['m']['z0'].z0) < 1e-6
    assert _rel(Sa['m']['dz'].dz, Sc['m']['dz'].dz) < 1e-6
    va, vc = np.array(Sa['m']['bias']['val']), np.array(Sc['m']['bias']['val'])
    assert np.any(vc != 0) and np.linalg.norm(va - vc) <= 1e-6 * np.linalg.norm(vc)
    with pytest.raises(NativeError):
        _bias_28(lsq_bias='eliminate', lsq_dense_max=0, lsq_cg_chunks=True)
