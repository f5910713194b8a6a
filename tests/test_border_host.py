"""Host side of compute_E with data and slope biases (smooth_fit's key lsq_E_border, the bordered
band order of lssurf_amd/errors.py): the column order handed to lsq_cov_band_bordered, the key's
validation and the refusals that stand with it — all before any device is touched."""
import numpy as np
import pytest

import lssurf_amd as LS
from conftest import golden, golden_kwargs, golden_points
from lssurf_amd.constraint_functions import reference_epoch_keep_cols
from lssurf_amd.errors import band_order, bordered_band_order
from priors_common import prior_kwargs


def _slope_kwargs(g):
    kw = golden_kwargs(g)
    kw['data_slope_sensors'] = np.array(kw['data_slope_sensors'])
    return kw


def _order_case(name, kw):
    g = golden(name)
    S = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, lsq_bias='columns', **kw(g))
    grids = S['grids']
    n_grid = int(grids['dz'].col_N)
    keep = reference_epoch_keep_cols(S['G_data'].col_N, grids['dz'], kw(g)['reference_epoch'])
    return S, grids, keep, n_grid


@pytest.mark.parametrize('name, kw, n_extra', [('sys_bias.npz', golden_kwargs, 18), ('sys_slope.npz', _slope_kwargs, None)])
def test_bordered_band_order(name, kw, n_extra):
    """Band part: band_order of the grid-only columns; border: the remaining kept columns, ascending."""
    S, grids, keep, n_grid = _order_case(name, kw)
    assert keep.size < S['G_data'].col_N            # a reference-epoch system: columns were removed
    n_bias = S['G_data'].col_N - n_grid
    assert n_bias > 0 and (n_extra is None or n_bias == n_extra)
    if name == 'sys_slope.npz':
        assert n_bias == golden(name)['bias_ID'].size + golden(name)['slope_val'].size
    perm, n_border = bordered_band_order(grids, keep, n_grid)
    assert n_border == n_bias == np.count_nonzero(keep >= n_grid)
    assert perm.dtype == np.int32 and np.array_equal(np.sort(perm), np.arange(keep.size))
    n_b = keep.size - n_border
    inside = keep[keep < n_grid]
    assert np.array_equal(perm[:n_b], band_order(grids, inside))   # compact ids of the grid columns come first
    assert np.array_equal(keep[perm[n_b:]], np.arange(n_grid, S['G_data'].col_N))
    assert np.all(keep[perm[:n_b]] < n_grid)
    # a system without border columns: the band order itself
    perm0, k0 = bordered_band_order(grids, inside, n_grid)
    assert k0 == 0 and np.array_equal(perm0, band_order(grids, inside))


def test_compute_E_with_biases_is_refused_without_the_key():
    g = golden('sys_bias.npz')
    kw = golden_kwargs(g)
    with pytest.raises(NotImplementedError, match='sigma_bias'):
        LS.smooth_fit(data=golden_points(g), **dict(kw, lsq_bias='auto', compute_E=True))
    with pytest.raises(NotImplementedError, match='sigma_bias'):
        LS.smooth_fit(data=golden_points(g), **dict(kw, lsq_bias='auto', compute_E=True, lsq_E_border=False))


def test_the_key_is_validated():
    g = golden('sys_bias.npz')
    kw = golden_kwargs(g)
    for bad in ('yes', 1, None):
        with pytest.raises(ValueError, match='lsq_E_border'):
            LS.smooth_fit(data=golden_points(g), **dict(kw, lsq_bias='auto', compute_E=True, lsq_E_border=bad))
    g0 = golden('sys_sf3d.npz')   # validated without biases too
    with pytest.raises(ValueError, match='lsq_E_border'):
        LS.smooth_fit(data=golden_points(g0), **dict(golden_kwargs(g0), lsq_E_border='yes'))


def test_refusals_that_stand_with_the_key(monkeypatch):
    """window method, sensor bias grids, priors and n_gpus = 2 stay refused with lsq_E_border=True,
    before a device system is made."""
    import sys
    sf = sys.modules['lssurf_amd.smooth_fit']

    def no_device(*a, **k):
        raise AssertionError('a device system was made')
    monkeypatch.setattr(sf, 'FitSystem', no_device)
    monkeypatch.setattr(sf, '_bias_fit_system', no_device)
    monkeypatch.setattr(sf, '_sgrid_fit_system', no_device)
    g = golden('sys_bias.npz')
    kw = dict(golden_kwargs(g), lsq_bias='auto', compute_E=True, lsq_E_border=True)
    with pytest.raises(NotImplementedError, match='window'):
        LS.smooth_fit(data=golden_points(g), **dict(kw, lsq_E_method='window'))
    with pytest.raises(NotImplementedError, match='one GPU'):
        LS.smooth_fit(data=golden_points(g), **dict(kw, n_gpus=2))
    gs = golden('sys_sgrid.npz')
    with pytest.raises(NotImplementedError, match='sensor_grid_bias_params'):
        LS.smooth_fit(data=golden_points(gs), **dict(golden_kwargs(gs), lsq_bias='columns', compute_E=True,
                                                      lsq_E_border=True))
    D = golden_points(gs)
    D.assign(sigma_corr=np.full(D.size, 0.5))
    with pytest.raises(NotImplementedError, match='sensor_grid_bias_params'):
        LS.smooth_fit(data=D, **dict(golden_kwargs(gs), bias_params=['sensor'], lsq_bias='columns', compute_E=True,
                                     lsq_E_border=True))
    gp = golden('sys_prior_dz.npz')
    with pytest.raises(NotImplementedError, match='prior'):
        LS.smooth_fit(data=golden_points(gp), **dict(prior_kwargs(gp), compute_E=True, lsq_E_border=True))
    Dp = golden_points(gp)
    Dp.assign(sigma_corr=np.full(Dp.size, 0.5))
    with pytest.raises(NotImplementedError, match='prior'):
        LS.smooth_fit(data=Dp, **dict(prior_kwargs(gp), bias_params=['sensor'], lsq_bias='columns', compute_E=True,
                                      lsq_E_border=True))


def test_window_refusal_in_calc_and_parse_errors_names_the_reason():
    from lssurf_amd.errors import WINDOW_BORDER_REFUSAL, calc_and_parse_errors
    assert 'couples' in WINDOW_BORDER_REFUSAL
    for method in ('window',):
        with pytest.raises(NotImplementedError, match='window'):
            calc_and_parse_errors({}, None, None, None, None, None, None, np.arange(4), {}, {}, method=method,
                                  bias_model={'bias_ID_dict': {0: {}}}, bias_params=['cycle'])
