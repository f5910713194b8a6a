"""Host side of the joint elimination of sensor bias grids beside data biases and slopes
(lsq_sgrid_joint; setup_sensor_grid_bias.joint_split) against what the reference recorded in
tests/golden/sys_sgrid_joint.npz (gen_golden_sgrid_joint.py)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import lssurf_amd as LS
from conftest import golden, golden_csr, golden_kwargs, golden_points
from lssurf_amd.bias_functions import assign_bias_ID
from lssurf_amd.constraint_functions import reference_epoch_keep_cols
from lssurf_amd.data_slope_bias import slope_columns
from lssurf_amd.setup_sensor_grid_bias import joint_split

NAMES = ['sensor_1.0_bias', 'sensor_2.0_bias', 'sensor_4.0_bias']
PARAMS = ['sensor', 'cycle']
N_ID, N_SLOPE, N_SG = 30, 6, 63 + 35 + 35


@functools.lru_cache(maxsize=None)
def joint_objects():
    """Host objects of the reference's recorded system: the operators without the eliminated terms
    (Sg), the full ones (Sf, which also hold the device form of the grids), the IDs and c, the slope
    groups, coefficients and c.  Shared with tests/test_gpu_sgrid_joint.py."""
    g = golden('sys_sgrid_joint.npz')
    kw = golden_kwargs(g)
    kw['data_slope_sensors'] = np.array(kw['data_slope_sensors'])
    kw_grid = {k: v for k, v in kw.items()
               if not k.startswith('bias_') and k not in ('data_slope_sensors', 'sensor_grid_bias_params')}
    Sg = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, **kw_grid)
    Sf = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, lsq_bias='columns', **kw)
    D, bm = assign_bias_ID(golden_points(g), PARAMS)
    expected = np.array([bm['E_bias'][j] for j in range(len(bm['E_bias']))])
    present, grp, u = slope_columns(D, kw['data_slope_sensors'])
    assert list(present) == list(g['slope_keys']) == [1., 2., 3.]
    cs = np.full((len(present), 2), 1. / (0.01 * 1000))
    assert Sf['sensor_grids']['names'] == NAMES
    return g, kw, Sg, Sf, D.bias_ID.astype(np.int32), 1. / expected, (grp, u, cs)


def test_the_split_reproduces_the_column_systems_normal_equations():
    """Z = [B_bias U_slope B_grid] and M = ZᵀW²Z + C from what Python hands the device, M block diagonal
    as joint_split says, and the reduced operator equal to the Schur complement of the reference's
    recorded A on its eliminated columns."""
    g, kw, Sg, Sf, ids, c, (grp, u, cs) = joint_objects()
    sg = Sf['sensor_grids']
    A = golden_csr(g).toarray()
    assert A.shape == (7237, 1339)
    n_e = N_ID + N_SLOPE + N_SG
    n_g = A.shape[1] - n_e
    assert c.size == N_ID and cs.size == N_SLOPE and int(sg['n_nodes'].sum()) == N_SG
    assert list(sg['n_nodes']) == [63, 35, 35] and list(sg['shift']) == [0., 0.25, 0.]
    split = joint_split(sg['grid'], ids, N_ID, grp, 3)
    sensor = Sf['data'].sensor
    # sensor 0: loose IDs; sensors 1, 2: six IDs, slopes and a grid; 3: IDs and slopes, loose; 4: six IDs and a grid
    assert [len(d) for d in split['dense']] == [8, 8, 6]
    assert list(split['grp_grid']) == [0, 1, -1]
    for j in range(N_ID):
        s = np.unique(sensor[ids == j])
        assert s.size == 1 and split['id_grid'][j] == {1.: 0, 2.: 1, 4.: 2}.get(float(s[0]), -1)
    # the operators without the eliminated columns, weighted
    keep = reference_epoch_keep_cols(Sg['G_data'].col_N, Sg['grids']['dz'], kw['reference_epoch'])
    assert keep.size == n_g
    Gg = sp.vstack([Sg['G_data'].toCSR(col_N=Sg['Gc'].col_N), Sg['Gc'].toCSR(col_N=Sg['Gc'].col_N)]).tocsr()[:, keep]
    wg = 1. / np.concatenate((Sg['Ed'], Sg['Ec']))
    Ag = sp.diags(wg).dot(Gg).toarray()
    n = Sg['data'].size
    Wd = wg[:n]
    # Z on the data rows and C
    Z = np.zeros((n, n_e))
    Z[np.arange(n), ids] = 1.
    on = np.flatnonzero(grp >= 0)
    for k in range(2):
        Z[on, N_ID + 2 * grp[on] + k] = u[on, k]
    off = np.concatenate([[0], np.cumsum(sg['n_nodes'])])
    rows = np.flatnonzero(sg['grid'] >= 0)
    for q in range(4):
        np.add.at(Z, (rows, N_ID + N_SLOPE + off[sg['grid'][rows]] + sg['node'][rows, q]), sg['wt'][rows, q])
    C = np.zeros((n_e, n_e))
    C[:N_ID, :N_ID] = np.diag(c ** 2)
    C[N_ID:N_ID + N_SLOPE, N_ID:N_ID + N_SLOPE] = np.diag(cs.ravel() ** 2)
    for s, (r, cc, v) in enumerate(sg['K']):
        np.add.at(C, (N_ID + N_SLOPE + off[s] + r, N_ID + N_SLOPE + off[s] + cc), v)
    ZW = Wd[:, None] * Z
    M = ZW.T @ ZW + C
    # block diagonal as claimed: a block per grid with its dense nodes; outside them the IDs couple to
    # their own group's slopes only
    owner = np.concatenate([split['id_grid'], np.repeat(split['grp_grid'], 2), np.repeat(np.arange(3), sg['n_nodes'])])
    for s in range(3):
        mine = owner == s
        assert not M[np.ix_(mine, ~mine)].any()
        assert mine.sum() == sg['n_nodes'][s] + len(split['dense'][s])
    loose = np.flatnonzero(owner < 0)
    loose_ids = loose[loose < N_ID]
    Ml = M[np.ix_(loose_ids, loose_ids)]
    assert not (Ml - np.diag(np.diag(Ml))).any()                        # a diagonal
    id_group = np.array([np.max(grp[ids == j], initial=-1) for j in range(N_ID)])
    for j in loose_ids:
        for q in range(3):
            if id_group[j] != q:
                assert not M[j, N_ID + 2 * q:N_ID + 2 * q + 2].any()     # and one 2 × 2 system per group
    # the reduced operator against the Schur complement of the recorded A
    rng = np.random.default_rng(5)
    p = rng.standard_normal(n_g)
    N = A.T @ A
    Ngg, Nge, Nee = N[:n_g, :n_g], N[:n_g, n_g:], N[n_g:, n_g:]
    ref = Ngg @ p - Nge @ np.linalg.solve(Nee, Nge.T @ p)
    Ad = Ag[:n]
    got = Ag.T @ (Ag @ p) - Ad.T @ (ZW @ np.linalg.solve(M, ZW.T @ (Ad @ p)))
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    assert err <= 1e-10, err
    assert np.linalg.norm(Ngg @ p - ref) / np.linalg.norm(ref) > 1e-3   # the elimination acts
    # the reference's column order: the biases, the slopes, the sensor grids, last
    assert np.allclose(M, Nee, rtol=1e-12, atol=1e-12 * np.abs(Nee).max())


def test_joint_split_refuses_what_is_not_nested():
    grid = np.array([0, 0, -1, 1, -1])
    with pytest.raises(ValueError, match='nested'):
        joint_split(grid, np.array([0, 0, 0, 1, 2]), 3)                 # ID 0 in grid 0 and outside
    with pytest.raises(ValueError, match='nested'):
        joint_split(grid, np.array([0, 0, 2, 0, 2]), 3)                 # ID 0 in two grids
    with pytest.raises(ValueError, match='nested'):
        joint_split(grid, np.array([0, 0, 2, 1, 2]), 3, np.array([0, -1, 0, -1, -1]), 1)   # a group likewise
    out = joint_split(grid, np.array([0, 0, 2, 1, 2]), 4, np.array([0, -1, 1, -1, 1]), 2)
    assert list(out['id_grid']) == [0, 1, -1, -1] and list(out['grp_grid']) == [0, -1]
    assert out['dense'] == [[('id', 0), ('slope_x', 0), ('slope_y', 0)], [('id', 1)]]


def test_the_new_key_and_the_unchanged_refusals():
    g = golden('sys_sgrid_joint.npz')
    kw = golden_kwargs(g)
    kw['data_slope_sensors'] = np.array(kw['data_slope_sensors'])
    pts = lambda: golden_points(g)   # noqa: E731
    for bad in (1, 'yes', None):
        with pytest.raises(ValueError, match='lsq_sgrid_joint'):
            LS.smooth_fit(data=pts(), lsq_bias='eliminate', lsq_sgrid_joint=bad, **kw)
    # without the key the three terms together stay refused
    with pytest.raises(NotImplementedError, match='bias_params'):
        LS.smooth_fit(data=pts(), lsq_bias='eliminate', **kw)
    # with it: priors, compute_E, n_gpus > 1, LSQR and the dense preconditioner stay refused
    for extra in (dict(prior_args={}), dict(compute_E=True), dict(compute_E=True, lsq_E_border=True), dict(n_gpus=2),
                  dict(lsq_method='lsqr'), dict(lsq_precond=2)):
        with pytest.raises(NotImplementedError):
            LS.smooth_fit(data=pts(), lsq_bias='eliminate', lsq_sgrid_joint=True, **dict(kw, **extra))
