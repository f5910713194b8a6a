"""Host side of the slope biases (lssurf_amd/data_slope_bias.py, smooth_fit's data_slope_sensors)
against what the reference recorded in tests/golden/sys_slope.npz (gen_golden_slope.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import lssurf_amd as LS
from conftest import golden, golden_csr, golden_kwargs, golden_points
from lssurf_amd.constraint_functions import reference_epoch_keep_cols
from lssurf_amd.data_slope_bias import data_slope_bias


def _kwargs(g):
    kw = golden_kwargs(g)
    kw['data_slope_sensors'] = np.array(kw['data_slope_sensors'])
    return kw


def test_fit_objects_assemble_the_references_matrix():
    """[G_data; Gc] of return_fit_objects, weighted by 1 / [Ed; Ec] and without the reference
    epoch's columns, is the matrix of the reference's first solve: same entries, same values."""
    g = golden('sys_slope.npz')
    kw = _kwargs(g)
    S = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, lsq_bias='columns', **kw)
    G_data, Gc = S['G_data'], S['Gc']
    assert G_data.col_N == Gc.col_N == g['m_all'].size
    n_slope = g['slope_val'].size
    assert n_slope == 4
    # rows: bias constraints, then slope constraints, last
    rows_b = np.asarray(Gc.TOC['rows']['constraint_data_bias'])
    rows_s = np.asarray(Gc.TOC['rows']['constraint_data_slope'])
    assert np.array_equal(rows_s, np.arange(Gc.N_eq - n_slope, Gc.N_eq))
    assert np.array_equal(rows_b, np.arange(Gc.N_eq - n_slope - 24, Gc.N_eq - n_slope))
    assert np.array_equal(S['Ec'][-n_slope:], np.full(n_slope, 0.01 * 1000))
    assert np.array_equal(S['Ec'][-n_slope - 24:-n_slope], g['bias_expected'])
    keep = reference_epoch_keep_cols(G_data.col_N, S['grids']['dz'], kw['reference_epoch'])
    G = sp.vstack([G_data.toCSR(col_N=Gc.col_N), Gc.toCSR(col_N=Gc.col_N)]).tocsr()[:, keep]
    w = 1. / np.concatenate((S['Ed'], S['Ec']))
    A = sp.diags(w).dot(G).tocsr()
    ref = golden_csr(g)
    assert A.shape == ref.shape == (6967, 1198)
    for M in (A, ref):
        M.sum_duplicates()
        M.eliminate_zeros()
        M.sort_indices()
    assert np.array_equal(A.indptr, ref.indptr) and np.array_equal(A.indices, ref.indices)
    # one product per entry on either side: at most an ulp apart
    assert np.allclose(A.data, ref.data, rtol=4e-16, atol=0)
    assert np.allclose(S['rhs'] * w, g['b'], rtol=4e-16, atol=0)


def test_slope_columns_are_centred_kilometres_per_sensor():
    g = golden('sys_slope.npz')
    D = golden_points(g)
    bm = {}
    G, Gc, bm = data_slope_bias(D, bm, col_0=100, sensors=np.array([1., 2., 7.]), E_rms_bias=0.01)
    assert list(bm['slope_bias_dict']) == [1., 2.]
    assert np.array_equal(bm['slope_bias_dict'][1.], [100, 101]) and np.array_equal(bm['slope_bias_dict'][2.], [102, 103])
    assert (G.col_0, G.col_N) == (100, 104) and Gc.name == 'constraint_data_slope'
    assert np.array_equal(Gc.expected, np.full(4, 10.)) and np.array_equal(Gc.prior, np.zeros(4))
    assert np.array_equal(Gc.toCSR(col_N=104)[:, 100:].toarray(), np.eye(4))
    U = sp.csr_matrix((G.v, (G.r, G.c)), shape=(D.size, 104)).toarray()[:, 100:]
    for k, s in enumerate((1., 2.)):
        mine = D.sensor == s
        assert np.array_equal(U[mine, 2 * k], (D.x[mine] - np.nanmean(D.x[mine])) / 1000)
        assert np.array_equal(U[mine, 2 * k + 1], (D.y[mine] - np.nanmean(D.y[mine])) / 1000)
        assert not U[~mine, 2 * k:2 * k + 2].any()


def test_no_listed_sensor_present_changes_nothing():
    g = golden('sys_slope.npz')
    D = golden_points(g)
    bm = {'E_bias': {}}
    assert data_slope_bias(D, bm, col_0=5, sensors=np.array([7., 9.])) == (None, None, bm)
    assert bm == {'E_bias': {}}
    kw = _kwargs(g)
    S0 = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, lsq_bias='columns',
                       **dict(kw, data_slope_sensors=None))
    S1 = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, lsq_bias='columns',
                       **dict(kw, data_slope_sensors=np.array([7., 9.])))
    assert S1['G_data'].col_N == S0['G_data'].col_N and S1['Gc'].N_eq == S0['Gc'].N_eq
    assert 'constraint_data_slope' not in S1['Gc'].TOC['rows']
    assert np.array_equal(S1['Ec'], S0['Ec'])


def test_slope_refusals():
    g = golden('sys_slope.npz')
    kw = _kwargs(g)
    pts = lambda: golden_points(g)   # noqa: E731
    with pytest.raises(NotImplementedError, match='lsq_bias'):
        LS.smooth_fit(data=pts(), **kw)
    with pytest.raises(NotImplementedError, match='lsq_bias'):
        LS.smooth_fit(data=pts(), **dict(kw, bias_params=None))
    with pytest.raises(ValueError, match='bias_params'):
        LS.smooth_fit(data=pts(), **dict(kw, bias_params=None, lsq_bias='auto'))
    for extra in (dict(compute_E=True), dict(n_gpus=2), dict(lsq_bias='eliminate', lsq_method='lsqr'),
                  dict(lsq_bias='eliminate', lsq_precond=2), dict(bias_edit_vals={'sensor': [1]}),
                  dict(lsq_bias='eliminate', prior_args={})):
        with pytest.raises(NotImplementedError):
            LS.smooth_fit(data=pts(), **dict(dict(kw, lsq_bias='auto'), **extra))
    with pytest.raises(ValueError, match='lsq_bias'):
        LS.smooth_fit(data=pts(), **dict(kw, lsq_bias='sometimes'))
