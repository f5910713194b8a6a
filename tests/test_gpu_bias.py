"""Data biases eliminated inside CGNR (lsq_set_data_bias; csrc/bias.inc) and smooth_fit's
bias_params through the solver key lsq_bias.

Operator: lsq_normal_apply with biases set must equal AᵀA p − A_dᵀ W Q W A_d p formed on the host from
the assembled A (Q = W B D⁻¹ Bᵀ W, D_j = Σ_{i∈j} W_i² + c_j²) to the normal operator's own tolerance,
1e-12 of max|q|, on the ID layouts that can break a segmented sum.  Solves: the reference's recorded
bias system (tests/golden/sys_bias.npz, gen_golden_bias.py) within the project's REL 1e-6 / ABS 1e-4;
smooth_fit against the reference's outputs with the tolerances of test_gpu_golden_sebin.py."""
import functools

import numpy as np
import pytest

import lssurf_amd as LS
from conftest import golden, golden_kwargs, golden_points
from lssurf_amd._native import NativeError
from lssurf_amd.bias_functions import assign_bias_ID
from lssurf_amd.constraint_functions import reference_epoch_keep_cols
from lssurf_amd.smooth_fit import FitSystem
from test_gpu_cgnr import _profiler_runs_real_iterations, _synthetic_system, _times_are_positive

pytestmark = pytest.mark.gpu
REL, ABS = 1e-6, 1e-4
TOL = dict(atol=1e-12, btol=1e-12, conlim=1e12)
PARAMS = ['sensor', 'cycle']
SEG_LENGTHS = [1, 63, 64, 65, 255, 256, 257]
LONG_RANK = 32 * 512 + 300   # points of an ID that spans more than 32 chunks wherever it starts


def _layouts(npts, keep, rng):
    """name -> (ids, c): the ID layouts of the operator test."""
    out = {'one': (np.zeros(npts, np.int32), np.array([3.0])),
           'each': (rng.permutation(npts).astype(np.int32), rng.uniform(1., 30., npts))}
    # segments of the critical lengths, the rest over 3 IDs; IDs dealt out by a random permutation of
    # the points, so no segment is contiguous in the solver's cell-sorted order
    nb = len(SEG_LENGTHS) + 3
    ids = np.empty(npts, np.int32)
    order = rng.permutation(npts)
    k = 0
    for j, n in enumerate(SEG_LENGTHS):
        ids[order[k:k + n]] = j
        k += n
    ids[order[k:]] = len(SEG_LENGTHS) + rng.integers(0, 3, npts - k)
    out['mixed'] = (ids, rng.uniform(1., 30., nb))
    # an ID all of whose rows are masked (its sum is 0, D = c²): the masked rows share ID 0
    ids_m = np.where(keep, 1 + rng.integers(0, 4, npts), 0).astype(np.int32)
    out['masked_id'] = (ids_m, rng.uniform(1., 30., 5))
    # an ID in [0, nb) that no point carries
    ids_e = rng.integers(0, 5, npts).astype(np.int32)
    ids_e[ids_e == 2] = 3
    out['empty_id'] = (ids_e, rng.uniform(1., 30., 5))
    if npts >= 2 * LONG_RANK + 2000:
        # ranks spread over more than 32 chunks of 512 index entries are summed by their whole wave:
        # two of them and four short ones in one wave (IDs 0 … 5), long and short interleaved, and a
        # last chunk that is not full
        ids_l = np.empty(npts, np.int32)
        order = rng.permutation(npts)
        cut = np.cumsum([LONG_RANK, 700, LONG_RANK + 513, 1, 65])
        for j, (a, b) in enumerate(zip(np.r_[0, cut], np.r_[cut, npts])):
            ids_l[order[a:b]] = j
        out['long'] = (ids_l, rng.uniform(1., 30., 6))
    return out


def _host_reduced(A, n_kept, Wk, idk, c, pc):
    """(AᵀA − A_dᵀ W Q W A_d) p from the assembled, weighted, row-selected A (data rows first)."""
    Ad = A[:n_kept]
    t = Ad @ pc                                               # W A_d p
    s = np.bincount(idk, weights=Wk * t, minlength=c.size)
    D = np.bincount(idk, weights=Wk ** 2, minlength=c.size) + c ** 2
    return A.T @ (A @ pc) - Ad.T @ (Wk * (s / D)[idk])


@pytest.mark.parametrize('which', ['t64', 'tdense'])
def test_reduced_normal_operator(gpu_available, which):
    S, fs, w, rhs = _synthetic_system(which)
    rng = np.random.default_rng(11)
    keep = rng.random(fs.n_data) > 0.2
    try:
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(np.concatenate([keep, np.ones(fs.n_con, bool)]))
        ok, why = fs.solver.cg_available(1)
        assert ok, why
        A = fs.solver.get_csr()          # before the biases are set: the grid operator
        Wk = w[:fs.n_data][keep]
        pc = rng.standard_normal(A.shape[1])
        pf = np.zeros(fs.n_full)
        pf[fs.keep_cols] = pc
        q_plain = fs.solver.normal_apply(pf)[fs.keep_cols]
        layouts = _layouts(fs.n_data, keep, rng)
        assert ('long' in layouts) == (which == 'tdense')
        for name, (ids, c) in layouts.items():
            fs.solver.set_data_bias(ids, c)
            ok, why = fs.solver.cg_available(1)
            assert ok, (name, why)
            q = fs.solver.normal_apply(pf)[fs.keep_cols]
            qr = _host_reduced(A, int(keep.sum()), Wk, ids[keep], c, pc)
            err = np.abs(q - qr).max() / np.abs(qr).max()
            print(f'{which} {name}: err {err:.2e}, correction {np.abs(q - q_plain).max() / np.abs(qr).max():.2e}')
            assert err <= 1e-12, (name, err)
            assert np.abs(q - q_plain).max() > 1e-9 * np.abs(qr).max(), name   # the biases did act
            assert np.array_equal(q, fs.solver.normal_apply(pf)[fs.keep_cols]), name   # run to run
    finally:
        fs.close()


def test_solves_are_bitwise_reproducible(gpu_available):
    S, fs, w, rhs = _synthetic_system('t64')
    rng = np.random.default_rng(12)
    keep = rng.random(fs.n_data) > 0.1
    ids, c = _layouts(fs.n_data, keep, rng)['mixed']
    try:
        fs.solver.set_data_bias(ids, c)
        out = []
        for _ in range(2):
            x = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
            out.append((x, fs.solver.data_bias(), fs.stats['iters']))
    finally:
        fs.close()
    assert fs.stats['method'] == 1
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2]
    assert np.any(out[0][1] != 0)


def test_clearing_the_biases_restores_every_bit(gpu_available):
    rng = np.random.default_rng(13)
    res = []
    for with_bias in (False, True):
        S, fs, w, rhs = _synthetic_system('t64')
        keep = np.random.default_rng(14).random(fs.n_data) > 0.1
        try:
            if with_bias:
                ids, c = _layouts(fs.n_data, keep, rng)['mixed']
                fs.solver.set_data_bias(ids, c)
                xb = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
                fs.solver.set_data_bias(None, None)
                with pytest.raises(NativeError):
                    fs.solver.data_bias()
            x = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
            pf = np.zeros(fs.n_full)
            pf[fs.keep_cols] = np.random.default_rng(15).standard_normal(fs.keep_cols.size)
            res.append((x, fs.solver.normal_apply(pf), fs.stats['iters']))
        finally:
            fs.close()
    assert np.any(xb != res[1][0])
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2]


def test_profile_cg_with_biases_runs_real_iterations(gpu_available):
    """profile_cg on the live state of iterate() with biases set: real steps (the same estimates after
    16 as plain iterations give), positive times, the byte figures of the model iterate() reports."""
    S, fs, w, rhs = _synthetic_system('t64')
    keep = np.random.default_rng(18).random(fs.n_data) > 0.1
    ids, c = _layouts(fs.n_data, keep, np.random.default_rng(19))['mixed']
    try:
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(np.concatenate([keep, np.ones(fs.n_con, bool)]))
        fs.solver.set_data_bias(ids, c)
        prof = _profiler_runs_real_iterations(fs.solver, rhs, fs.n_data, lambda reps: fs.solver.profile_cg(reps=reps),
                                              lambda: fs.solver.set_data_bias(ids, c))
        _times_are_positive([prof[k] for k in ('cg_data', 'cg_normal', 'cg_update', 'cg_scalars')])
        with_bias = fs.solver.iterate(rhs, 1, precond=3, method=1, b_rows=fs.n_data)['bytes_per_iter']
        assert sum(prof['bytes'].values()) == with_bias
        fs.solver.set_data_bias(None, None)
        assert with_bias > fs.solver.iterate(rhs, 1, precond=3, method=1, b_rows=fs.n_data)['bytes_per_iter']
    finally:
        fs.close()


@functools.lru_cache(maxsize=None)
def _bias_objects(name='bias'):
    """Host objects of the reference's recorded bias system: the grid-only operators, the full
    ones, IDs and c."""
    g = golden(f'sys_{name}.npz')
    kw = golden_kwargs(g)
    kw_grid = {k: v for k, v in kw.items() if not k.startswith('bias_')}
    Sg = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, **kw_grid)
    Sf = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, lsq_bias='columns', **kw)
    D, bm = assign_bias_ID(golden_points(g), PARAMS)
    expected = np.array([bm['E_bias'][j] for j in range(len(bm['E_bias']))])
    return g, kw, Sg, Sf, D.bias_ID.astype(np.int32), 1. / expected


def _weights_rhs(S):
    w = 1. / np.concatenate((S['Ed'], S['Ec']))
    rhs = np.zeros(w.size)
    rhs[:S['data'].size] = S['data'].z
    return w, rhs


def test_eliminated_solve_reaches_the_oracle(gpu_available):
    g, kw, Sg, Sf, ids, c = _bias_objects()
    xs = g['x']
    n_grid = xs.size - c.size
    keep = reference_epoch_keep_cols(Sg['G_data'].col_N, Sg['grids']['dz'], kw['reference_epoch'])
    assert keep.size == n_grid
    w, rhs = _weights_rhs(Sg)
    ran = []
    fs = FitSystem(Sg['G_data'], Sg['Gc'], keep, Sg['Gc'].col_N, grids=Sg['grids'], bias=(ids, c))
    try:
        for precond in (1, 3, 4):
            if not fs.solver.cg_available(precond)[0]:
                continue
            x = fs.solve(w, np.ones(fs.n_data, bool), rhs, precond=precond, method=1, maxit=200000, **TOL)
            b = fs.solver.data_bias()
            ran.append(precond)
            assert fs.stats['method'] == 1 and fs.stats['istop'] in (1, 2), (precond, fs.stats)
            eg = np.linalg.norm(x - xs[:n_grid]) / np.linalg.norm(xs[:n_grid])
            eb = np.linalg.norm(b - xs[n_grid:]) / np.linalg.norm(xs[n_grid:])
            print(f'precond {precond}: {fs.stats["iters"]} iterations, grid {eg:.2e}, biases {eb:.2e}')
            assert eg <= REL and np.max(np.abs(x - xs[:n_grid])) <= ABS, (precond, eg)
            assert eb <= 1e-6, (precond, eb)
            x_el = np.concatenate([x, b])
            assert np.array_equal(fs.expand(x)[fs.n_full:], b)
    finally:
        fs.close()
    assert 1 in ran and 3 in ran, ran
    # the in-project cross-check: the biases as ordinary columns, dense preconditioner
    keep_f = reference_epoch_keep_cols(Sf['G_data'].col_N, Sf['grids']['dz'], kw['reference_epoch'])
    wf, rhsf = _weights_rhs(Sf)
    fc = FitSystem(Sf['G_data'], Sf['Gc'], keep_f, Sf['Gc'].col_N, grids=Sf['grids'])
    try:
        assert fc.formation == 'coo'
        x_col = fc.solve(wf, np.ones(fc.n_data, bool), rhsf, precond=2, method=0, **TOL)
    finally:
        fc.close()
    assert np.linalg.norm(x_col - x_el) / np.linalg.norm(x_col) <= 1e-8


def test_warm_start_after_a_mask_change(gpu_available):
    S, fs, w, rhs = _synthetic_system('t64')
    rng = np.random.default_rng(16)
    keep1 = rng.random(fs.n_data) > 0.1
    keep2 = keep1 & (rng.random(fs.n_data) > 0.05)
    ids, c = _layouts(fs.n_data, keep1, rng)['mixed']
    w2 = w * np.where(np.arange(w.size) < fs.n_data, rng.uniform(0.5, 2, w.size), 1.0)
    try:
        fs.solver.set_data_bias(ids, c)
        x1 = fs.solve(w2, keep1, rhs, precond=3, method=1, **TOL)
        xw = fs.solve(w2, keep2, rhs, x0=x1, precond=3, method=1, **TOL)
        bw, it_warm = fs.solver.data_bias(), fs.stats['iters']
        xc = fs.solve(w2, keep2, rhs, precond=3, method=1, **TOL)
        bc, it_cold = fs.solver.data_bias(), fs.stats['iters']
        xj = fs.solve(w2, keep2, rhs, x0=x1, precond=1, method=1, **TOL)
    finally:
        fs.close()
    assert np.linalg.norm(xw - xc) / np.linalg.norm(xc) <= 1e-8
    assert np.linalg.norm(xj - xc) / np.linalg.norm(xc) <= 1e-8
    assert np.linalg.norm(bw - bc) / np.linalg.norm(bc) <= 1e-8
    assert it_warm < it_cold


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    ok = np.isfinite(b)
    return np.linalg.norm(a[ok] - b[ok]) / max(np.linalg.norm(b[ok]), 1e-300)


def _check_fit_against_reference(S, g, name):
    d, m = S['data'], S['m']
    flips = int(np.sum(d.three_sigma_edit != g['data_three_sigma_edit'].astype(bool)))
    assert flips == 0
    assert _rel(d.sigma_extra, g['data_sigma_extra']) < 1e-5
    assert _rel(m['z0'].z0, g['z0']) < 1e-6
    assert _rel(m['dz'].dz, g['dz']) < 1e-6
    assert _rel(d.z_est, g['data_z_est']) < 1e-6
    bias = m['bias']
    assert list(bias.keys()) == [str(k) for k in g['bias_keys']]
    assert np.array_equal(bias['ID'], g['bias_ID']) and np.array_equal(bias['expected'], g['bias_expected'])
    for p in PARAMS:
        assert np.array_equal(bias[p], g['bias_' + p])
    assert np.linalg.norm(np.array(bias['val']) - g['bias_val']) <= 1e-6 * np.linalg.norm(g['bias_val'])
    assert np.array_equal(bias['N_raw'], g['bias_N_raw']) and np.array_equal(bias['N_edited'], g['bias_N_edited'])
    # the IDs edit_by_bias removed: the fit's own flags against the reference's bias_param_dict['edited']
    pd = S['bias_model']['bias_param_dict']
    assert pd['ID'] == [int(j) for j in g['bias_ID']]
    edited = np.asarray(pd.get('edited', np.zeros(len(pd['ID']), bool)), dtype=bool)
    assert np.array_equal(edited, g['bias_edited'])
    if name == 'bias_edit':
        assert edited.any() and not edited.all()
        assert not np.any(d.three_sigma_edit[np.isin(d.bias_ID, np.array(pd['ID'])[edited])])
        # left with their constraint row alone, their biases vanish (to the tolerance of 'val' above)
        assert np.all(np.abs(np.array(bias['val'])[edited]) <= 1e-6 * np.linalg.norm(g['bias_val']))
    assert m['all'].size == g['m_all'].size
    assert np.array_equal(m['all'][-len(bias['val']):], bias['val'])   # the biases behind the grids' columns
    assert 'constraint_data_bias' in S['TOC']['rows']


@pytest.mark.parametrize('mode', ['eliminate', 'columns'])
@pytest.mark.parametrize('name', ['bias', 'bias_edit'])
def test_smooth_fit_with_biases_matches_reference(gpu_available, name, mode):
    g = golden(f'sys_{name}.npz')
    kw = golden_kwargs(g)
    extra = dict(lsq_bias='eliminate', lsq_dense_max=0) if mode == 'eliminate' else dict(lsq_bias='columns')
    S = LS.smooth_fit(data=golden_points(g), **kw, **extra)
    _check_fit_against_reference(S, g, name)
    assert S['timing']['lsq_last']['method'] == (1 if mode == 'eliminate' else 0)


# the fixture has 1 170 kept grid unknowns and 18 biases (1 188 columns with them)
@pytest.mark.parametrize('extra, method, precond', [
    (dict(lsq_bias='eliminate'), 1, (3,)),                       # default options: no dense preconditioner
    (dict(lsq_bias='eliminate', lsq_precond=4), 1, (4,)),
    (dict(lsq_bias='auto'), 0, (2,)),                            # small: columns, dense
    (dict(lsq_bias='auto', lsq_dense_max=1180), 0, (1, 3)),      # grid unknowns ≤ the limit < all columns
    (dict(lsq_bias='auto', lsq_dense_max=1169), 1, (3,)),        # one below the grid unknowns: eliminate
    (dict(lsq_bias='auto', lsq_dense_max=0, lsq_method='lsqr'), 0, (1, 3)),
])
def test_smooth_fit_bias_modes_and_preconditioners(gpu_available, extra, method, precond):
    g = golden('sys_bias_edit.npz')
    S = LS.smooth_fit(data=golden_points(g), **golden_kwargs(g), **extra)
    _check_fit_against_reference(S, g, 'bias_edit')
    last = S['timing']['lsq_last']
    assert last['method'] == method and last['precond'] in precond, last


def test_a_second_matrix_is_refused_and_the_biases_stay(gpu_available):
    """A handle takes one matrix: biases cannot outlive the points they index."""
    S, fs, w, rhs = _synthetic_system('t64')
    rng = np.random.default_rng(18)
    keep = rng.random(fs.n_data) > 0.1
    ids, c = _layouts(fs.n_data, keep, rng)['mixed']
    pf = np.zeros(fs.n_full)
    pf[fs.keep_cols] = rng.standard_normal(fs.keep_cols.size)
    try:
        fs.solver.set_data_bias(ids, c)
        x = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
        q = fs.solver.normal_apply(pf)
        gdesc, interp, coords, stencils, npts, fields = fs.desc
        half = tuple(None if v is None else np.ascontiguousarray(v[:npts // 2]) for v in coords)
        for pts, n in ((coords, npts), (half, npts // 2)):
            with pytest.raises(NativeError, match='already set'):
                fs.solver.set_matrix_stencil(fs.n_data + fs.n_con, fs.n_full, gdesc, interp, pts, stencils, n)
        assert np.array_equal(fs.solver.normal_apply(pf), q)
        assert np.array_equal(fs.solve(w, keep, rhs, precond=3, method=1, **TOL), x)
    finally:
        fs.close()


def test_refusals_leave_the_handle_usable(gpu_available):
    S, fs, w, rhs = _synthetic_system('t64')
    keep = np.ones(fs.n_data, bool)
    rng = np.random.default_rng(17)
    ids, c = _layouts(fs.n_data, keep, rng)['mixed']
    try:
        x0 = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
        with pytest.raises(NativeError, match='outside'):
            fs.solver.set_data_bias(np.where(np.arange(ids.size) == 5, c.size, ids), c)
        with pytest.raises(NativeError, match='outside'):
            fs.solver.set_data_bias(np.where(np.arange(ids.size) == 7, -1, ids), c)
        for bad in (0.0, -1.0, np.nan):
            cb = c.copy()
            cb[3] = bad
            with pytest.raises(NativeError, match='> 0'):
                fs.solver.set_data_bias(ids, cb)
        with pytest.raises(NativeError, match='npts'):
            fs.solver.set_data_bias(ids[:-1], c)
        with pytest.raises(NativeError):
            fs.solver.data_bias()          # none set
        # nothing was set by the refused calls: the same bits as before
        assert np.array_equal(fs.solve(w, keep, rhs, precond=3, method=1, **TOL), x0)
        fs.solver.set_data_bias(ids, c)
        with pytest.raises(NativeError, match='no lsq_solve'):
            fs.solver.data_bias()          # set, not solved
        with pytest.raises(NativeError, match='CGNR'):
            fs.solve(w, keep, rhs, precond=3, method=0, **TOL)
        for precond in (2, 5):
            with pytest.raises(NativeError, match='precond'):
                fs.solve(w, keep, rhs, precond=precond, method=1, **TOL)
            ok, why = fs.solver.cg_available(precond)
            assert not ok and why
        xb = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
        assert fs.stats['method'] == 1 and np.any(fs.solver.data_bias() != 0)
        assert np.any(xb != x0)
    finally:
        fs.close()
