"""Host side of compute_E with biases at window scale (smooth_fit's key lsq_E_border_solve,
errors.split_border): the split of the fit objects that lsq_cov_border_solved takes against the blocks
of the golden matrix's AᵀA, the key's validation and the refusals that stand with it — all before any
device is touched."""
import numpy as np
import pytest
import scipy.sparse as sp

import lssurf_amd as LS
from conftest import golden, golden_csr, golden_kwargs, golden_points
from lssurf_amd.constraint_functions import reference_epoch_keep_cols
from lssurf_amd.errors import split_border
from priors_common import prior_kwargs


def _slope_kwargs(g):
    kw = golden_kwargs(g)
    kw['data_slope_sensors'] = np.array(kw['data_slope_sensors'])
    return kw


@pytest.mark.parametrize('name, kw', [('sys_bias.npz', golden_kwargs), ('sys_slope.npz', _slope_kwargs)])
def test_split_border_gives_the_blocks_of_the_golden_normal_matrix(name, kw):
    """BᵗW²B + c_con = (AᵀA)[border, border] and A_gᵀW²B = (AᵀA)[grid, border] of the golden A
    (the reference's weighted matrix over the kept columns: the golden's own weights 1 / [Ed; Ec]),
    the blocks sliced from the golden matrix with scipy."""
    g = golden(name)
    S = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, lsq_bias='columns', **kw(g))
    grids = S['grids']
    n_grid = int(grids['dz'].col_N)
    keep = reference_epoch_keep_cols(S['G_data'].col_N, grids['dz'], kw(g)['reference_epoch'])
    n_g = int(np.count_nonzero(keep < n_grid))
    k = keep.size - n_g
    A = golden_csr(g)
    assert A.shape == (S['G_data'].N_eq + S['Gc'].N_eq, keep.size) and k > 0
    M = (A.T @ A).tocsr()
    M_bb, M_gb = M[n_g:, n_g:].toarray(), M[:n_g, n_g:].toarray()

    G_grid, Gc_grid, B, c_con = split_border(S['G_data'], S['Gc'], S['Ec'], keep, n_grid)
    nd = int(S['G_data'].N_eq)
    assert B.shape == (nd, k) and c_con.shape == (k, k)
    assert sp.isspmatrix_csc(B) and B.has_sorted_indices
    assert G_grid.N_eq == nd and G_grid.col_N == n_grid and Gc_grid.col_N == n_grid
    # the bias (and slope) constraint rows: one per border column, behind the grid-only prefix
    assert Gc_grid.N_eq == S['Gc'].N_eq - k
    w_d = 1. / np.asarray(S['Ed'], float)
    W2 = sp.diags(w_d ** 2)
    C = (B.T @ W2 @ B).toarray() + c_con
    Ag = G_grid.toCSR(row_N=nd, col_N=n_grid).tocsc()[:, keep[:n_g]]
    AgB = (Ag.T @ W2 @ B).toarray()
    for mine, ref, what in ((C, M_bb, 'border block'), (AgB, M_gb, 'coupling block')):
        d = np.abs(mine - ref).max() / np.abs(ref).max()
        print(f'{name} {what}: {d:.2e}')
        assert d <= 1e-12, (what, d)
    # the grid-only rows: the golden's grid block from the split's two operators
    w_c = 1. / np.asarray(S['Ec'], float)[:Gc_grid.N_eq]
    Acg = Gc_grid.toCSR(row_N=int(Gc_grid.N_eq), col_N=n_grid).tocsc()[:, keep[:n_g]]
    N = (Ag.T @ W2 @ Ag + Acg.T @ sp.diags(w_c ** 2) @ Acg).toarray()
    M_gg = M[:n_g, :n_g].toarray()
    assert np.abs(N - M_gg).max() / np.abs(M_gg).max() <= 1e-12


def test_split_border_checks_the_prefix_and_the_grid_ops():
    g = golden('sys_bias.npz')
    S = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, lsq_bias='columns', **golden_kwargs(g))
    n_grid = int(S['grids']['dz'].col_N)
    keep = reference_epoch_keep_cols(S['G_data'].col_N, S['grids']['dz'], golden_kwargs(g)['reference_epoch'])
    # grid-only operators of another size are not taken for this system's
    S0 = LS.smooth_fit(data=golden_points(golden('sys_sf3d.npz')), return_fit_objects=True,
                       **golden_kwargs(golden('sys_sf3d.npz')))
    with pytest.raises(ValueError, match='grid_ops'):
        split_border(S['G_data'], S['Gc'], S['Ec'], keep, n_grid, grid_ops=(S0['G_data'], S0['Gc']))
    # the fit's own grid-only operators (the same call without biases) are returned as they are
    kw = {k: v for k, v in golden_kwargs(g).items() if k != 'bias_params'}
    Sg = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, **kw)
    G_grid, Gc_grid, B, c_con = split_border(S['G_data'], S['Gc'], S['Ec'], keep, n_grid,
                                             grid_ops=(Sg['G_data'], Sg['Gc']))
    assert G_grid is Sg['G_data'] and Gc_grid is Sg['Gc'] and Gc_grid.parts is not None


def test_the_key_is_validated():
    g = golden('sys_bias.npz')
    kw = golden_kwargs(g)
    for bad in ('yes', 1, None):
        with pytest.raises(ValueError, match='lsq_E_border_solve'):
            LS.smooth_fit(data=golden_points(g), **dict(kw, lsq_bias='auto', compute_E=True, lsq_E_border=True,
                                                        lsq_E_border_solve=bad))
    g0 = golden('sys_sf3d.npz')   # validated without biases too
    with pytest.raises(ValueError, match='lsq_E_border_solve'):
        LS.smooth_fit(data=golden_points(g0), **dict(golden_kwargs(g0), lsq_E_border_solve='yes'))
    assert LS.smooth_fit.__globals__['DEFAULTS']['lsq_E_border_solve'] is False


def test_without_lsq_E_border_the_first_refusal_stands():
    g = golden('sys_bias.npz')
    kw = golden_kwargs(g)
    for extra in ({}, {'lsq_E_border': False}, {'lsq_E_method': 'window'}):
        with pytest.raises(NotImplementedError, match='sigma_bias'):
            LS.smooth_fit(data=golden_points(g), **dict(kw, lsq_bias='auto', compute_E=True, lsq_E_border_solve=True,
                                                        **extra))


def test_refusals_that_stand_with_the_key(monkeypatch):
    """sensor bias grids, priors and n_gpus = 2 stay refused with lsq_E_border_solve=True, before a
    device system is made; without the key the window refusal keeps its words."""
    import sys
    sf = sys.modules['lssurf_amd.smooth_fit']

    def no_device(*a, **k):
        raise AssertionError('a device system was made')
    monkeypatch.setattr(sf, 'FitSystem', no_device)
    monkeypatch.setattr(sf, '_bias_fit_system', no_device)
    monkeypatch.setattr(sf, '_sgrid_fit_system', no_device)
    g = golden('sys_bias.npz')
    on = dict(compute_E=True, lsq_E_border=True, lsq_E_border_solve=True, lsq_E_method='window')
    kw = dict(golden_kwargs(g), lsq_bias='auto', **on)
    with pytest.raises(NotImplementedError, match='one GPU'):
        LS.smooth_fit(data=golden_points(g), **dict(kw, n_gpus=2))
    from lssurf_amd.errors import WINDOW_BORDER_REFUSAL
    with pytest.raises(NotImplementedError) as e:
        LS.smooth_fit(data=golden_points(g), **dict(kw, lsq_E_border_solve=False))
    assert str(e.value) == 'smooth_fit: ' + WINDOW_BORDER_REFUSAL
    gs = golden('sys_sgrid.npz')
    with pytest.raises(NotImplementedError, match='sensor_grid_bias_params'):
        LS.smooth_fit(data=golden_points(gs), **dict(golden_kwargs(gs), lsq_bias='columns', **on))
    D = golden_points(gs)
    D.assign(sigma_corr=np.full(D.size, 0.5))
    with pytest.raises(NotImplementedError, match='sensor_grid_bias_params'):
        LS.smooth_fit(data=D, **dict(golden_kwargs(gs), bias_params=['sensor'], lsq_bias='columns', **on))
    gp = golden('sys_prior_dz.npz')
    with pytest.raises(NotImplementedError, match='prior'):
        LS.smooth_fit(data=golden_points(gp), **dict(prior_kwargs(gp), **on))
    Dp = golden_points(gp)
    Dp.assign(sigma_corr=np.full(Dp.size, 0.5))
    with pytest.raises(NotImplementedError, match='prior'):
        LS.smooth_fit(data=Dp, **dict(prior_kwargs(gp), bias_params=['sensor'], lsq_bias='columns', **on))


def test_calc_and_parse_errors_keeps_its_refusal_without_the_keyword():
    from lssurf_amd.errors import calc_and_parse_errors
    with pytest.raises(NotImplementedError, match='window'):
        calc_and_parse_errors({}, None, None, None, None, None, None, np.arange(4), {}, {}, method='window',
                              bias_model={'bias_ID_dict': {0: {}}}, bias_params=['cycle'], border_solve=False)


def test_split_border_reads_only_the_trailing_operators_of_a_stacked_Gc(monkeypatch):
    """With the fit's grid-only operators at hand the split must not materialise the constraint rows
    of the grids (7·10⁷ rows at C4): the same B and c_con as from all of Gc's triplets."""
    g = golden('sys_slope.npz')
    kw = _slope_kwargs(g)
    S = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, lsq_bias='columns', **kw)
    n_grid = int(S['grids']['dz'].col_N)
    keep = reference_epoch_keep_cols(S['G_data'].col_N, S['grids']['dz'], kw['reference_epoch'])
    _, _, B0, c0 = split_border(S['G_data'], S['Gc'], S['Ec'], keep, n_grid)
    Sg = LS.smooth_fit(data=golden_points(g), return_fit_objects=True,
                       **{k: v for k, v in kw.items() if k not in ('bias_params', 'data_slope_sensors')})
    S = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, lsq_bias='columns', **kw)   # nothing materialised yet

    def no_triplets():
        raise AssertionError("all of Gc's triplets were formed")
    monkeypatch.setattr(S['Gc'], 'triplets', no_triplets)
    _, Gc_grid, B, c_con = split_border(S['G_data'], S['Gc'], S['Ec'], keep, n_grid, grid_ops=(Sg['G_data'], Sg['Gc']))
    assert Gc_grid is Sg['Gc'] and Sg['Gc'].materialized is False
    assert (B != B0).nnz == 0 and np.array_equal(c_con, c0)
