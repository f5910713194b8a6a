"""Host side of the data biases (lssurf_amd/bias_functions.py) against what the reference recorded
in tests/golden/sys_bias.npz (gen_golden_bias.py): IDs, expected values and parameter columns."""
import numpy as np
import pytest

import lssurf_amd as LS
from conftest import golden, golden_kwargs, golden_points
from lssurf_amd import containers as pc
from lssurf_amd.bias_functions import assign_bias_ID, parse_biases, setup_bias_fit
from lssurf_amd.lin_op import lin_op

PARAMS = ['sensor', 'cycle']


@pytest.mark.parametrize('name', ['bias', 'bias_edit'])
def test_ids_expected_and_parameters_match_the_reference(name):
    g = golden(f'sys_{name}.npz')
    assert g['data_bias_ID'].size == g['in_x'].size   # every input point took part in the fit
    D, bm = assign_bias_ID(golden_points(g), PARAMS)
    assert np.array_equal(D.bias_ID, g['data_bias_ID'])
    ids = list(bm['bias_ID_dict'])
    assert np.array_equal(ids, g['bias_ID'])
    assert np.array_equal([bm['E_bias'][j] for j in ids], g['bias_expected'])
    for p in PARAMS:
        assert np.array_equal([bm['bias_ID_dict'][j][p] for j in ids], g['bias_' + p])
        assert np.array_equal(bm['bias_param_dict'][p], g['bias_' + p])
    assert bm['bias_param_dict']['ID'] == ids


def test_setup_bias_fit_appends_columns_and_constraints():
    g = golden('sys_bias.npz')
    D, bm = assign_bias_ID(golden_points(g), PARAMS)
    G = lin_op(name='stub', col_0=0, col_N=7).data_bias(np.arange(D.size), col=np.zeros(D.size, int))
    ops = []
    setup_bias_fit(D, bm, G, ops, bias_param_name='bias_ID')
    assert G.col_N == 7 + 18 and len(ops) == 1 and ops[0].name == 'constraint_data_bias'
    assert np.array_equal(ops[0].expected, g['bias_expected'])
    A = G.toCSR()
    assert np.array_equal(A[:, 7:].toarray().argmax(axis=1), D.bias_ID.astype(int))
    assert [bm['bias_ID_dict'][j]['col'] for j in range(18)] == list(range(7, 25))
    m = np.arange(25.)
    b, _ = parse_biases(m, bm, PARAMS)
    assert list(b) == PARAMS + ['val', 'ID', 'expected'] and b['val'] == list(m[7:])


def test_nan_parameters_share_one_id_and_come_back_as_nan():
    sensor = np.array([1., np.nan, 1., np.nan, 0., np.nan])
    cycle = np.array([2., 5., 2., 5., 2., 5.])
    D = pc.data().from_dict({'z': np.zeros(6), 'sensor': sensor, 'cycle': cycle,
                             'sigma_corr': np.array([1., 2., 3., 4., 5., np.nan])})
    D, bm = assign_bias_ID(D, PARAMS)
    ids = D.bias_ID
    assert ids[1] == ids[3] == ids[5] and ids[0] == ids[2] and len(set(ids)) == 3
    nan_id = int(ids[1])
    assert np.isnan(bm['bias_ID_dict'][nan_id]['sensor']) and bm['bias_ID_dict'][nan_id]['cycle'] == 5.
    assert bm['E_bias'][nan_id] == 3.0            # nanmedian of (2, 4, NaN)
    assert nan_id == 0                            # −9999 sorts first, as in the reference's ordering


def test_zero_expected_bias_raises():
    D = pc.data().from_dict({'z': np.zeros(4), 'sensor': np.array([0., 0., 1., 1.]),
                             'sigma_corr': np.array([0., 0., 1., 1.])})
    D, bm = assign_bias_ID(D, ['sensor'])
    G = lin_op(name='stub', col_0=0, col_N=3).data_bias(np.arange(4), col=np.zeros(4, int))
    with pytest.raises(ValueError):
        setup_bias_fit(D, bm, G, [], bias_param_name='bias_ID')


def test_bias_params_without_lsq_bias_still_refused():
    g = golden('sys_bias.npz')
    kw = golden_kwargs(g)
    with pytest.raises(NotImplementedError, match='lsq_bias'):
        LS.smooth_fit(data=golden_points(g), **kw)
    for extra in (dict(compute_E=True), dict(n_gpus=2), dict(lsq_bias='eliminate', lsq_method='lsqr'),
                  dict(lsq_bias='eliminate', lsq_precond=2), dict(bias_edit_vals={'sensor': [1]})):
        with pytest.raises(NotImplementedError):
            LS.smooth_fit(data=golden_points(g), **dict(dict(kw, lsq_bias='auto'), **extra))


def test_fit_objects_carry_the_bias_columns_and_constraint_rows_last():
    g = golden('sys_bias.npz')
    S = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, lsq_bias='eliminate', **golden_kwargs(g))
    Gc = S['Gc']
    rows = np.asarray(Gc.TOC['rows']['constraint_data_bias'])
    assert np.array_equal(rows, np.arange(Gc.N_eq - 18, Gc.N_eq))
    assert S['G_data'].col_N == Gc.col_N == g['m_all'].size
    assert np.array_equal(S['Ec'][-18:], g['bias_expected'])
