"""GPU parity of compute_E with data and slope biases: the bordered band factor
(lsq_cov_band_bordered, lssurf_amd/csrc/border.inc) and smooth_fit(lsq_E_border=True).

The shared system is tests/test_gpu_band.py::_small_system's recipe on a 17 × 17 × 6 grid (1734 grid
columns = 27.09 tiles: ragged, several tile rows, a band of w ≥ 2 tiles so the ring wraps) with 2·17²
points, a `cycle` field dealt out as permutation % k, sigma_corr 0.5 and 10 % of the data rows
masked.  Border sizes: a single column, less than one panel of 64, exactly one, one past it, three
ragged panels, and a mixed border of 130 biases + 2 × 2 slope columns.

* E = sqrt(diag((AᵀA)⁻¹)) against a host float64 inverse (1e-9, the bound of test_gpu_band.py for
  this comparison; the host float64 run of the same bordered formula sits at ≤ 1e-12) and against
  the device dense factor (1e-10, the project's band-vs-dense bound), over all columns and over the
  band and the border columns apart;
* the border acts (> 1e-3 against the band-only window factor), a second call returns the same
  bits, re-weighting scales E, n_border = 0 is cov_band bit for bit;
* op rows over the band columns against op·R⁻¹ of the dense factor;
* malformed calls and a border block that is not positive definite raise NativeError and leave the
  handle usable;
* smooth_fit(compute_E=True, lsq_E_border=True) on sys_bias / sys_slope: 'eliminate' and 'columns',
  'band' and 'dense' agree within 1e-10, and with the reference's own uncertainties where
  tests/golden/sys_bias_E.npz records them."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import lssurf_amd as LS
from conftest import golden, golden_kwargs, golden_points
from lssurf_amd._native import LSQ_BORDER_MAX, NativeError
from lssurf_amd.errors import bordered_band_order

pytestmark = pytest.mark.gpu

S_NODES, NT = 17, 6
N_GRID_KEPT = S_NODES * S_NODES * NT          # z0 + dz without the reference epoch
CASES = [1, 5, 64, 65, 130, 'mixed']


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _build(k):
    """(fit objects, FitSystem, weights, row mask, perm, n_border) of one case"""
    from lssurf_amd import synthetic
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    from lssurf_amd.smooth_fit import FitSystem
    S, nt = S_NODES, NT
    W = {'x': (S - 1) * 100., 'y': (S - 1) * 100., 't': (nt - 1) * 0.25}
    rng = np.random.default_rng(7)
    npts = 2 * S * S
    x, y = (rng.random(npts) - 0.5) * W['x'], (rng.random(npts) - 0.5) * W['y']
    t = (rng.random(npts) - 0.5) * W['t']
    z = 10 * np.sin(2 * np.pi * x / (W['x'] / 2)) + rng.normal(0, 0.1, npts)
    fields = {'x': x, 'y': y, 'time': t, 'z': z, 'sigma': np.full(npts, 0.1), 'sigma_corr': np.full(npts, 0.5)}
    kw = dict(bias_params=['cycle'])
    if k == 'mixed':
        cycle = (rng.permutation(npts) % 130).astype(float)
        fields.update(cycle=cycle, sensor=cycle % 3)
        kw = dict(bias_params=['cycle', 'sensor'], data_slope_sensors=np.array([1., 2.]))
    else:
        fields.update(cycle=(rng.permutation(npts) % k).astype(float))
    D = LS.containers.data().from_dict(fields)
    out = LS.smooth_fit(data=D, W=W, ctr={'x': 0., 'y': 0., 't': 0.}, spacing={'z0': 100., 'dz': 100., 'dt': 0.25},
                        E_RMS=dict(synthetic.E_RMS_NOTEBOOK), reference_epoch=nt // 2, return_fit_objects=True,
                        lsq_bias='columns', **kw)
    keep_cols = reference_epoch_keep_cols(out['G_data'].col_N, out['grids']['dz'], nt // 2)
    fs = FitSystem(out['G_data'], out['Gc'], keep_cols, out['Gc'].col_N)
    w = 1. / np.concatenate((out['Ed'], out['Ec']))
    keep = np.random.default_rng(3).random(fs.n_data) > 0.1
    mask = np.concatenate([keep, np.ones(fs.n_con, bool)])
    perm, n_border = bordered_band_order(out['grids'], keep_cols, int(out['grids']['dz'].col_N))
    assert n_border == (134 if k == 'mixed' else k) and perm.size - n_border == N_GRID_KEPT
    return out, fs, w, mask, perm, n_border


@functools.lru_cache(maxsize=None)
def _case(k):
    """every device result of one border size, and the host inverse, computed once"""
    out, fs, w, mask, perm, nb = _build(k)
    r = {'perm': perm, 'n_border': nb, 'n': perm.size}
    try:
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(mask)
        r['E'], _, r['info'] = fs.solver.cov_band_bordered(perm, nb)
        r['E_again'], _, _ = fs.solver.cov_band_bordered(perm, nb)
        r['E_dense'] = fs.solver.sigma_x()
        A = fs.solver.get_csr()
        r['E_window'], _, _ = fs.solver.cov_band_window(perm[:perm.size - nb])
        fs.solver.set_row_weight(w * 1.5)
        r['E_rw'], _, _ = fs.solver.cov_band_bordered(perm, nb)
    finally:
        fs.close()
    r['E_host'] = np.sqrt(np.diag(np.linalg.inv((A.T @ A).toarray())))
    return r


@pytest.mark.parametrize('k', CASES)
def test_bordered_sigma_matches_host_inverse_and_dense(gpu_available, k):
    r = _case(k)
    band, border = r['perm'][:r['n'] - r['n_border']], r['perm'][r['n'] - r['n_border']:]
    for name, sel in (('all', slice(None)), ('band', band), ('border', border)):
        host, dense = _rel(r['E'][sel], r['E_host'][sel]), _rel(r['E'][sel], r['E_dense'][sel])
        print(f'k={k} {name}: vs host inverse {host:.2e}, vs dense {dense:.2e}')
        assert host <= 1e-9, (k, name, host)
        assert dense <= 1e-10, (k, name, dense)
    info = r['info']
    assert info[6] == -(-r['n_border'] // 64) * 64 and info[7] > 0 and info[9] > 0
    assert info[1] == 28 and info[0] >= 2, info          # 27.09 tiles; the ring wraps


@pytest.mark.parametrize('k', CASES)
def test_border_acts_repeats_and_reweights(gpu_available, k):
    r = _case(k)
    band = r['perm'][:r['n'] - r['n_border']]
    moved = np.abs(r['E'][band] - r['E_window']).max() / np.abs(r['E_window']).max()
    print(f'k={k}: the border moves the band sigma by {moved:.2e}')
    assert moved > 1e-3, moved
    assert np.array_equal(r['E'], r['E_again'])
    assert _rel(r['E_rw'] * 1.5, r['E']) <= 1e-10


def test_no_border_is_cov_band_bit_for_bit(gpu_available):
    out, fs, w, mask, perm, nb = _build(5)
    try:
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(mask)
        op = sp.csr_matrix((np.array([1., -2., 0.5]), (np.array([0, 0, 2]), np.array([3, 40, 7]))), shape=(3, perm.size))
        E0, oe0, info0 = fs.solver.cov_band(perm, op)
        E1, oe1, info1 = fs.solver.cov_band_bordered(perm, 0, op)
    finally:
        fs.close()
    assert np.array_equal(E0, E1) and np.array_equal(oe0, oe1)
    assert np.array_equal(info0[:4], info1[:4]) and not info1[6:].any()


def _op_rows(perm, n_b, rng):
    """the 300 rows of test_band_op_rows_in_and_out_of_band, drawn over the band columns only"""
    band = perm[:n_b]
    rows, cols, vals = [], [], []
    for i in range(300):
        if i % 3 == 0:      # local: a few columns near one position (inside the band)
            c0 = rng.integers(0, n_b - 20)
            cc = band[c0 + rng.choice(20, 4, replace=False)]
        elif i % 3 == 1:    # wide: columns far apart (outside the band)
            cc = band[rng.choice(n_b, 6, replace=False)]
        else:               # single column
            cc = band[rng.choice(n_b, 1)]
        rows += [i] * cc.size
        cols += list(cc)
        vals += list(rng.standard_normal(cc.size))
    return sp.csr_matrix((vals, (rows, cols)), shape=(300, perm.size))


def test_op_rows_over_the_band_columns(gpu_available):
    out, fs, w, mask, perm, nb = _build(65)
    op = _op_rows(perm, perm.size - nb, np.random.default_rng(9))
    try:
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(mask)
        E, oe, info = fs.solver.cov_band_bordered(perm, nb, op)
        Ri = fs.solver.rinv()
    finally:
        fs.close()
    ref = np.sqrt(((op @ Ri) ** 2).sum(axis=1)).ravel()
    print(f'op rows vs op·R⁻¹: {_rel(oe, ref):.2e}')
    assert _rel(oe, ref) <= 1e-10, _rel(oe, ref)
    assert _rel(E, _case(65)['E']) == 0.0      # E does not depend on the op rows


def test_malformed_calls_raise_and_leave_the_handle_usable(gpu_available):
    out, fs, w, mask, perm, nb = _build(5)
    n = perm.size
    E_ref = _case(5)['E']
    try:
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(mask)

        def still_answers():
            E, _, _ = fs.solver.cov_band(perm)     # the whole matrix as one (full) band
            assert _rel(E, E_ref) <= 1e-9

        op = sp.csr_matrix((np.array([1., 1.]), (np.array([0, 0]), np.array([perm[0], perm[n - 1]]))), shape=(1, n))
        with pytest.raises(NativeError, match='border column'):
            fs.solver.cov_band_bordered(perm, nb, op)
        still_answers()
        twice = perm.copy()
        twice[n - 1] = twice[0]
        with pytest.raises(NativeError, match='permutation'):
            fs.solver.cov_band_bordered(twice, nb)
        twice = perm.copy()
        twice[1] = twice[0]
        with pytest.raises(NativeError, match='permutation'):
            fs.solver.cov_band_bordered(twice, nb)
        still_answers()
        with pytest.raises(NativeError):
            fs.solver.cov_band_bordered(perm, LSQ_BORDER_MAX + 1)
        with pytest.raises(NativeError):
            fs.solver.cov_band_bordered(perm, -1)
        still_answers()
    finally:
        fs.close()


def test_border_block_not_positive_definite(gpu_available):
    """One ID without a kept data row and with a zero-weight constraint row: its column of A is
    zero, the Schur complement's pivot is not positive, and the call says which block failed."""
    out, fs, w, mask, perm, nb = _build(5)
    E_ref = _case(5)['E']
    the_id = 2
    rows = np.asarray(out['Gc'].TOC['rows']['constraint_data_bias'])
    w0, mask0 = w.copy(), mask.copy()
    w0[fs.n_data + rows[the_id]] = 0.
    mask0[:fs.n_data] &= np.asarray(out['data'].bias_ID) != the_id
    try:
        fs.solver.set_row_weight(w0)
        fs.solver.set_row_mask(mask0)
        with pytest.raises(NativeError, match='border'):
            fs.solver.cov_band_bordered(perm, nb)
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(mask)
        E, _, _ = fs.solver.cov_band_bordered(perm, nb)
    finally:
        fs.close()
    assert np.array_equal(E, E_ref)


def _slope_kwargs(g):
    kw = golden_kwargs(g)
    kw['data_slope_sensors'] = np.array(kw['data_slope_sensors'])
    return kw


@functools.lru_cache(maxsize=None)
def _fits(name):
    """smooth_fit(compute_E=True, lsq_E_border=True) of a golden system: {(lsq_bias, lsq_E_method): out}"""
    g = golden(name)
    kw = _slope_kwargs(g) if 'slope' in name else golden_kwargs(g)
    combos = [('eliminate', 'band'), ('columns', 'band'), ('eliminate', 'dense'), ('columns', 'dense')]
    if 'slope' in name:
        combos = [('eliminate', 'band'), ('columns', 'dense')]
    return {c: LS.smooth_fit(data=golden_points(g), compute_E=True, lsq_E_border=True, lsq_bias=c[0],
                             lsq_E_method=c[1], **kw) for c in combos}


def _grid_sigmas(E):
    return {k: getattr(v, k) for k, v in E.items() if k not in ('sigma_bias', 'sigma_slope_bias')}


@pytest.mark.parametrize('name', ['sys_bias.npz', 'sys_slope.npz'])
def test_smooth_fit_compute_E_with_biases(gpu_available, name):
    fits = _fits(name)
    first = next(iter(fits))
    ref = fits[first]
    Er = ref['E']
    assert {'sigma_z0', 'sigma_dz', 'sigma_bias', 'sigma_slope_bias'} <= set(Er)
    assert set(Er['sigma_bias']) == set(ref['m']['bias'])
    n_bias = len(ref['m']['bias']['val'])
    n_slope = 2 * len(ref['m']['slope_bias'])
    assert np.all(np.asarray(Er['sigma_bias']['val']) > 0)
    if 'slope' in name:
        assert n_slope > 0 and set(Er['sigma_slope_bias']) == set(ref['m']['slope_bias'])
        for v in Er['sigma_slope_bias'].values():
            assert v['slope_x'] > 0 and v['slope_y'] > 0
    else:
        assert Er['sigma_slope_bias'] == {}
    for c, out in fits.items():
        if c[1] == 'band':
            assert out['timing']['E_band']['border'] == n_bias + n_slope
            assert out['timing']['E_band']['border_bytes'] > 0
        E = out['E']
        assert set(E) == set(Er)
        a, b = _grid_sigmas(E), _grid_sigmas(Er)
        for key in b:
            ok = np.isfinite(b[key])
            assert np.array_equal(ok, np.isfinite(a[key])), (c, key)
            d = _rel(a[key][ok], b[key][ok])
            print(f'{name} {c} {key}: {d:.2e}')
            assert d <= 1e-10, (c, key, d)
        for key in Er['sigma_bias']:
            x, y = np.asarray(E['sigma_bias'][key], float), np.asarray(Er['sigma_bias'][key], float)
            assert np.allclose(x, y, rtol=1e-10, atol=0, equal_nan=True), (c, key)
        for sk, v in Er['sigma_slope_bias'].items():
            for comp in ('slope_x', 'slope_y'):
                assert abs(E['sigma_slope_bias'][sk][comp] - v[comp]) <= 1e-10 * abs(v[comp]), (c, sk, comp)


def test_smooth_fit_sigma_matches_the_reference(gpu_available):
    """Against the reference's compute_E on the sys_bias configuration: 1e-8 against its result with
    an exact R⁻¹ (the bound of test_gpu_smooth_fit.py), and 10 × the recorded difference against
    its own result, which drops |R⁻¹| ≤ 1e-5."""
    g = golden('sys_bias_E.npz')
    out = _fits('sys_bias.npz')[('eliminate', 'band')]
    E = out['E']
    ours = {'sigma_z0': E['sigma_z0'].sigma_z0, 'sigma_dz': E['sigma_dz'].sigma_dz,
            'sigma_bias': np.asarray(E['sigma_bias']['val'], float)}
    trunc = float(g['trunc_rel_diff'])
    for key, val in ours.items():
        ex, rf = g['Eexact_' + key], g['Eref_' + key]
        ok = np.isfinite(ex)
        d_ex, d_rf = _rel(val[ok], ex[ok]), _rel(val[ok], rf[ok])
        print(f'{key}: vs exact {d_ex:.2e}, vs the reference {d_rf:.2e} (recorded truncation {trunc:.2e})')
        assert d_ex <= 1e-8, (key, d_ex)
        assert d_rf <= 10 * trunc, (key, d_rf, trunc)
