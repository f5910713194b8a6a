"""Host side of the dz priors (lssurf_amd/match_priors.py) against what the reference recorded in
tests/golden/sys_prior_edge.npz and sys_prior_dz.npz (gen_golden_prior.py): the prior rows, their
σ and priors, the selection rules, and what smooth_fit refuses."""
import numpy as np
import pytest
import scipy.sparse as sp

import lssurf_amd as LS
from conftest import golden, golden_points
from lssurf_amd import containers as pc
from lssurf_amd.assemble import describe, extra_rows_of
from lssurf_amd.match_priors import make_prior_op, match_prior_dz, match_tile_edges
from priors_common import golden_tiles, prior_kwargs, prior_rows


def _fit_objects(g, **extra):
    return LS.smooth_fit(data=golden_points(g), return_fit_objects=True, **dict(prior_kwargs(g), **extra))


def _weighted_reduced(op, grids, ref_epoch):
    """(1/expected)·G[:, kept columns] and prior/expected of one prior operator, as the reference
    forms them: TCinv·G·Ip_c by scipy products"""
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    keep = reference_epoch_keep_cols(op.col_N, grids['dz'], ref_epoch)
    G = op.toCSR(row_N=op.N_eq)
    W = sp.dia_matrix((1. / np.ravel(op.expected), 0), shape=(op.N_eq, op.N_eq))
    Ip_c = sp.coo_matrix((np.ones(keep.size), (keep, np.arange(keep.size))), shape=(op.col_N, keep.size)).tocsc()
    A = sp.csr_matrix(W.dot(G.tocoo()).dot(Ip_c))
    A.sum_duplicates()
    A.sort_indices()
    A.eliminate_zeros()
    return A, W.dot(np.ravel(op.prior))


@pytest.mark.parametrize('name', ['prior_edge', 'prior_dz'])
def test_prior_rows_sigma_and_priors_match_the_reference_bit_for_bit(name):
    g = golden(f'sys_{name}.npz')
    S = _fit_objects(g)
    grids, Gc = S['grids'], S['Gc']
    kw = prior_kwargs(g)
    if name == 'prior_edge':
        ops, xy = match_tile_edges(grids, kw['reference_epoch'], **kw['prior_edge_args'])
        assert sorted(xy) == ['E-1_N0', 'E0_N1', 'E1_N0']   # the far tile and the tile itself are skipped
    else:
        ops = match_prior_dz(grids, **kw['prior_args'])
    A_ref, b_ref = prior_rows(g)
    assert sum(op.N_eq for op in ops) == A_ref.shape[0] == int(g['n_prior'])
    # the points at the reference time dropped out: 4 of the 5 saved epochs remain
    tiles = golden_tiles(g)
    assert all(op.N_eq % 4 == 0 for op in ops) and all(t.t.size == 5 for t in tiles.values())
    blocks = [_weighted_reduced(op, grids, kw['reference_epoch']) for op in ops]
    A = sp.vstack([a for a, _ in blocks]).tocsr()
    A.sort_indices()
    Ar = sp.csr_matrix(A_ref)
    Ar.eliminate_zeros()
    assert np.array_equal(A.indptr, Ar.indptr) and np.array_equal(A.indices, Ar.indices)
    assert np.array_equal(A.data, Ar.data)
    assert np.array_equal(np.concatenate([b for _, b in blocks]), b_ref)
    # smooth_fit keeps them last in Gc, and Ec carries sigma_scale · sigma_dz there
    assert extra_rows_of(Gc) == A_ref.shape[0]
    assert np.array_equal(S['Ec'][-A_ref.shape[0]:], np.concatenate([np.ravel(op.expected) for op in ops]))
    if name == 'prior_dz':   # sigma_scale = 2
        pts = tiles['prior']
        assert np.array_equal(np.sort(ops[0].expected), np.sort(2. * pts.sigma_dz[:, :, [0, 1, 3, 4]].ravel()))


def test_describe_keeps_the_structured_description_of_the_other_rows():
    g = golden('sys_prior_edge.npz')
    S = _fit_objects(g)
    plain = LS.smooth_fit(data=golden_points(g), return_fit_objects=True,
                          **{k: v for k, v in prior_kwargs(g).items() if k != 'prior_edge_args'})
    assert describe(S['G_data'], S['Gc'], with_fields=True) is None            # priors are no stencil rows
    d = describe(S['G_data'], S['Gc'], with_fields=True, extra_rows=True)
    d0 = describe(plain['G_data'], plain['Gc'], with_fields=True)
    assert d is not None and d0 is not None
    assert d[4] == d0[4] and len(d[3]) == len(d0[3])
    for a, b in zip(d[3], d0[3]):
        assert (a.grid, a.row0, a.n_eq, a.ntpl) == (b.grid, b.row0, b.n_eq, b.ntpl)
    assert S['Gc'].N_eq == plain['Gc'].N_eq + int(g['n_prior'])


def _unit_grid():
    x = np.arange(-300., 301., 100.)
    t = np.array([-0.5, -0.125, 0.25, 0.625])   # uniform: the bounds are centre ± half-width (match_priors.py:85-92)
    shape = (x.size, x.size, t.size)
    rng = np.random.default_rng(3)
    return pc.grid.data().from_dict({'x': x, 'y': x.copy(), 't': t, 'dz': rng.normal(size=shape),
                                     'sigma_dz': 0.1 + rng.random(shape)})


def _unit_grids():
    g = golden('sys_prior_edge.npz')
    return _fit_objects(g)['grids']


def test_match_prior_dz_crop_skip_and_edge_pad():
    grids = _unit_grids()   # ±800 m, t −0.625 … 0.625
    d = _unit_grid()
    op, = match_prior_dz(grids, dzs=[d], ref_epoch=1)
    assert op.N_eq == 7 * 7 * 3   # every node, the reference epoch dropped
    assert np.array_equal(np.ravel(op.prior), d.dz[:, :, [0, 2, 3]].ravel())
    op, = match_prior_dz(grids, dzs=[d], ref_epoch=1, edge_pad={'xy': 100., 't': 0})
    assert op.N_eq == 5 * 5 * 3   # the outer ring of nodes is cropped
    assert np.array_equal(np.ravel(op.prior), d.dz[1:-1, 1:-1, :][:, :, [0, 2, 3]].ravel())
    # the reference's skip: np.arange(skip / 2, n, dtype=int) starts at int(skip / 2) with step 1
    op, = match_prior_dz(grids, dzs=[d], ref_epoch=1, skip={'xy': 2, 't': 1})
    assert op.N_eq == 6 * 6 * 3
    assert np.array_equal(np.ravel(op.prior), d.dz[1:, 1:, :][:, :, [0, 2, 3]].ravel())
    # a grid wider than the fit is cropped to the fit's bounds
    wide = pc.grid.data().from_dict({'x': np.arange(-1200., 1201., 400.), 'y': np.arange(-1200., 1201., 400.),
                                     't': d.t, 'dz': np.zeros((7, 7, 4)), 'sigma_dz': np.ones((7, 7, 4))})
    op, = match_prior_dz(grids, dzs=[wide], ref_epoch=1)
    assert op.N_eq == 5 * 5 * 3   # −800 … 800
    assert match_prior_dz(grids, dzs=[None]) == []


def test_make_prior_op_rows_are_the_difference_of_two_interpolations():
    grids = _unit_grids()
    pts = pc.data().from_dict({'x': np.array([10., 10., 250.]), 'y': np.array([-40., -40., 90.]),
                               'time': np.array([0.3, -0.125, 0.3]), 'dz': np.array([1., 2., 3.]),
                               'sigma_dz': np.array([.1, .2, .3])})
    op = make_prior_op(grids, pts, 'unit', ref_time=-0.125, sigma_scale=3)
    assert op.N_eq == 2 and np.array_equal(op.prior, [1., 3.]) and np.array_equal(op.expected, 3 * np.array([.1, .3]))
    assert np.allclose(op.toCSR(row_N=2).sum(axis=1), 0., atol=1e-15)   # weights of 1 minus weights of 1
    assert op.parts == [dict(kind='extra', row0=0, n_eq=2)]


def test_b_rows_ignores_prior_ops_on_the_device_path(monkeypatch):
    g = golden('sys_prior_edge.npz')
    seen = {}

    class Stop(Exception):
        pass

    class FakeSystem:
        def __init__(self, G_data, Gc, keep_cols, n_full, device=0, grids=None, extra_ops=None, **k):
            seen['n_extra'] = sum(op.N_eq for op in extra_ops)
            seen['n_data'] = G_data.N_eq
            self.n_extra = seen['n_extra']

        def __setattr__(self, k, v):
            object.__setattr__(self, k, v)
            if k == 'b_rows':
                seen['b_rows'] = v
                raise Stop

        def close(self):
            pass

    import sys
    sf = sys.modules['lssurf_amd.smooth_fit']
    monkeypatch.setattr(sf, 'FitSystem', FakeSystem)
    with pytest.raises(Stop):
        LS.smooth_fit(data=golden_points(g), **prior_kwargs(g))
    assert seen['n_extra'] == int(g['n_prior']) and seen['b_rows'] == seen['n_data'] == int(g['n_data'])


def test_refusals():
    g = golden('sys_prior_edge.npz')
    kw = prior_kwargs(g)
    for extra in (dict(compute_E=True), dict(n_gpus=2), dict(devices=[0, 0])):
        with pytest.raises(NotImplementedError, match='prior'):
            LS.smooth_fit(data=golden_points(g), **dict(kw, **extra))
    grids = _unit_grids()
    with pytest.raises(NotImplementedError, match='h5'):
        match_prior_dz(grids, filenames=['saved.h5'])
    with pytest.raises(NotImplementedError, match='prior_dir'):
        match_tile_edges(grids, 2, prior_dir='/tiles')
    gd = golden('sys_prior_dz.npz')
    with pytest.raises(NotImplementedError, match='prior'):
        LS.smooth_fit(data=golden_points(gd), **dict(prior_kwargs(gd), compute_E=True))


def test_priors_with_eliminated_biases_are_refused():
    """the third refusal: the device rows of lsq_bias='eliminate' are a prefix of the host rows, and
    the priors stand behind the bias constraint rows"""
    g = golden('sys_prior_edge.npz')
    D = golden_points(g)
    D.assign(sensor=(np.arange(D.size) % 3).astype(float), sigma_corr=np.full(D.size, 0.5))
    with pytest.raises(NotImplementedError, match="lsq_bias='eliminate'"):
        LS.smooth_fit(data=D, **dict(prior_kwargs(g), bias_params=['sensor'], lsq_bias='eliminate'))
