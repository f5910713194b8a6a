"""Sensor bias grids beside data biases and slopes, eliminated jointly inside CGNR
(lsq_set_sensor_grids_joint; csrc/sgrid.inc).

With Z = [B_bias U_slope B_grid] and M = ZᵀW²Z + C, lsq_normal_apply must equal
AᵀA p − A_dᵀ W Z M⁻¹ Zᵀ W A_d p formed densely on the host from the assembled, weighted, row-selected A,
to the normal operator's own tolerance, 1e-12 of max|q|.  The host asserts that M is block diagonal as
the device assumes (one block per grid with the bias IDs and slope groups inside it; the others on the
bias / slope path) and that every block's cond is ≤ 1e6, so the tolerance means something.  The
constraint weights c of the biases and slopes are a multiple of the median row weight, which keeps
the blocks' conds of the order the lattice-only layouts of test_gpu_sgrid.py have."""
import numpy as np
import pytest

from lssurf_amd._native import NativeError
from test_gpu_cgnr import _synthetic_system
from test_gpu_sgrid import _dense_B, _dense_K, _layout, _layouts   # which build on _cells and _K

pytestmark = pytest.mark.gpu
TOL = dict(atol=1e-12, btol=1e-12, conlim=1e12)
MAX_DENSE = 16
CLEAR = (None, None, None, None, None)


def _bias_part(grid, rng, per_grid=1, n_loose=3, groups=(), loose_group=False):
    """IDs and slope groups nested in the grids of `grid`: per_grid IDs inside every grid (dealt out at
    random, every ID with a row), n_loose IDs over the rows outside; a slope group on every grid of
    `groups`, and (loose_group) one over the rows of the first loose ID.  -> (ids, nb, grp, u, ngrp)"""
    ng = int(grid.max()) + 1
    per = per_grid if np.ndim(per_grid) else [per_grid] * ng
    ids = np.zeros(grid.size, np.int32)
    nb = 0
    for s in range(ng):
        rows = np.flatnonzero(grid == s)
        k = np.arange(rows.size) % per[s] if rows.size else np.zeros(0, int)
        ids[rows] = nb + rng.permutation(k)
        nb += per[s]
    loose = np.flatnonzero(grid < 0)
    ids[loose] = nb + rng.integers(0, n_loose, loose.size)
    grp = np.full(grid.size, -1, np.int32)
    for q, s in enumerate(groups):
        grp[grid == s] = q
    ngrp = len(groups)
    if loose_group:
        grp[(grid < 0) & (ids == nb)] = ngrp
        ngrp += 1
    u = rng.standard_normal((grid.size, 2))
    return ids, nb + n_loose, grp, u, ngrp


def _joint_layouts(which, npts, keep, rng):
    """name -> (sensor-grid layout, (ids, nb, grp, u, ngrp))"""
    out = {}
    if which == 'tdense':
        # (g) one claimed ID over the 20 000-row grid of the 'long' layout
        lay = _layouts(npts, keep, rng)['long']
        assert np.sum(lay[0] == 1) == 20000
        out['long'] = (lay, _bias_part(lay[0], rng, groups=(2,)))
        return out
    # (a) grids of 63, 64, 65 and 2 lattice nodes, each with one ID and one slope group: blocks of 66, 67, 68 and 5
    lay = _layouts(npts, keep, rng)['sizes']
    assert list(lay[3]) == [63, 64, 65, 2]
    out['sizes'] = (lay, _bias_part(lay[0], rng, groups=(0, 1, 2, 3)))
    # (b) exactly 16 dense nodes (14 IDs and a group); 63 lattice nodes and one ID: 64, no padding
    lay = _layout(npts, [(7, 9), (7, 9)], [900, 700], rng, edge=40)
    out['cap'] = (lay, _bias_part(lay[0], rng, per_grid=[14, 1], groups=(0,)))
    # (c) loose IDs and a loose group beside claimed ones; loose ranks of 0, 1, 63, 64 and 65 rows
    lay = _layout(npts, [(4, 6), (5, 5)], [600, 500], rng)
    ids, nb, grp, u, ngrp = _bias_part(lay[0], rng, groups=(0,))
    loose = rng.permutation(np.flatnonzero(lay[0] < 0))
    counts = [0, 1, 63, 64, 65]
    ids[loose] = 2 + len(counts)
    ids[loose[:sum(counts)]] = 2 + np.repeat(np.arange(len(counts)), counts)
    nb = 2 + len(counts) + 1
    grp[lay[0] < 0] = -1
    grp[(ids == 4) | (ids == 5)] = 1                 # the ranks of 63 and 64 rows form the loose group
    assert [int(np.sum(ids == 2 + k)) for k in range(5)] == counts
    out['loose'] = (lay, (ids, nb, grp, u, 2))
    # (d) a claimed ID all of whose rows are masked, and an ID in [0, nb) that no row carries
    lay = _layout(npts, [(5, 6), (3, 4)], [800, 400], rng)
    ids, nb, grp, u, ngrp = _bias_part(lay[0], rng, per_grid=[2, 1], groups=(0,))
    g0 = lay[0] == 0
    ids[g0] = np.where(keep[g0], 0, 1)
    assert np.any(ids == 1) and not np.any(keep[ids == 1])
    out['masked_id'] = (lay, (ids, nb + 1, grp, u, ngrp))
    # (e) a grid whose rows carry no slope beside one that does
    lay = _layout(npts, [(4, 5), (6, 4)], [700, 600], rng)
    out['one_slope'] = (lay, _bias_part(lay[0], rng, groups=(1,)))
    # (f) every row outside every grid
    lay = _layouts(npts, keep, rng)['none']
    ids = rng.integers(0, 5, npts).astype(np.int32)
    out['none'] = (lay, (ids, 5, np.where(ids < 2, ids, -1).astype(np.int32), rng.standard_normal((npts, 2)), 2))
    return out


def _host_blocks(layout, bias, keep, Wk, cb, cg):
    """(ZW, M, label per column of Z): Z = [B_bias U_slope B_grid] on the kept rows, M = ZᵀW²Z + C.
    A column's label names the block the device puts it into."""
    grid, node, wt, n_nodes, K = layout
    ids, nb, grp, u, ngrp = bias
    n = int(keep.sum())
    Bb = np.zeros((n, nb))
    Bb[np.arange(n), ids[keep]] = 1.
    U = np.zeros((n, 2 * ngrp))
    on = np.flatnonzero(grp[keep] >= 0)
    for k in range(2):
        U[on, 2 * grp[keep][on] + k] = u[keep][on, k]
    Bg, off = _dense_B(grid[keep], node[keep], wt[keep], n_nodes)
    ZW = Wk[:, None] * np.hstack([Bb, U, Bg])
    C = np.zeros((ZW.shape[1],) * 2)
    C[:nb, :nb] = np.diag(np.asarray(cb) ** 2)
    C[nb:nb + 2 * ngrp, nb:nb + 2 * ngrp] = np.diag(np.ravel(cg) ** 2)
    C[nb + 2 * ngrp:, nb + 2 * ngrp:] = _dense_K(n_nodes, K, off)
    M = ZW.T @ ZW + C
    # owners from all rows, kept or not
    def owner(rows):
        g = np.unique(grid[rows])
        assert g.size <= 1, 'the layout is not nested'
        return int(g[0]) if g.size else -1
    glab = []
    for q in range(ngrp):
        s = owner(grp == q)
        glab.append(('grid', s) if s >= 0 else ('group', q))
    lab = []
    for j in range(nb):
        s = owner(ids == j)
        q = np.unique(grp[(ids == j) & (grp >= 0)])
        lab.append(('grid', s) if s >= 0 else (glab[int(q[0])] if q.size else ('id', j)))
    for q in range(ngrp):
        lab += [glab[q]] * 2
    for s in range(n_nodes.size):
        lab += [('grid', s)] * int(n_nodes[s])
    return ZW, M, lab


def _host_reduced(A, n_kept, ZW, M, lab, pc):
    """((AᵀA − A_dᵀ W Z M⁻¹ Zᵀ W A_d) p, cond per block); asserts that M is block diagonal by label."""
    keys = sorted(set(lab))
    code = np.array([keys.index(k) for k in lab])
    assert not (M * (code[:, None] != code[None, :])).any()      # block diagonal as claimed
    conds = [np.linalg.cond(M[np.ix_(code == k, code == k)]) for k in range(len(keys))]
    Ad = A[:n_kept]
    sol = np.linalg.solve(M, ZW.T @ (Ad @ pc))
    return A.T @ (A @ pc) - Ad.T @ (ZW @ sol), conds


def _set_bias(fs, bias, cb, cg):
    ids, nb, grp, u, ngrp = bias
    fs.solver.set_data_bias(ids, cb)
    if ngrp:
        fs.solver.set_data_slope(grp, u, cg)


def _c(bias, w, n_data):
    """c of the biases and of the slopes: three times the median row weight"""
    c0 = 3. * float(np.median(w[:n_data]))
    return np.full(bias[1], c0), np.full((max(bias[4], 1), 2), c0)[:bias[4]]


@pytest.mark.parametrize('which', ['t64', 'tdense'])
def test_reduced_normal_operator(gpu_available, which):
    S, fs, w, rhs = _synthetic_system(which)
    rng = np.random.default_rng(41)
    keep = rng.random(fs.n_data) > 0.2
    try:
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(np.concatenate([keep, np.ones(fs.n_con, bool)]))
        ok, why = fs.solver.cg_available(1)
        assert ok, why
        A = fs.solver.get_csr()          # before anything is set: the grid operator
        n_kept = int(keep.sum())
        Wk = w[:fs.n_data][keep]
        pc = rng.standard_normal(A.shape[1])
        pf = np.zeros(fs.n_full)
        pf[fs.keep_cols] = pc
        layouts = _joint_layouts(which, fs.n_data, keep, rng)
        assert list(layouts) == (['long'] if which == 'tdense' else ['sizes', 'cap', 'loose', 'masked_id', 'one_slope', 'none'])
        for name, (layout, bias) in layouts.items():
            tag = f'{which} {name}'
            cb, cg = _c(bias, w, fs.n_data)
            _set_bias(fs, bias, cb, cg)
            q_bs = fs.solver.normal_apply(pf)[fs.keep_cols]      # biases and slopes, no grids
            fs.solver.set_sensor_grids(*layout, joint=True)
            ok, why = fs.solver.cg_available(1)
            assert ok, (tag, why)
            q = fs.solver.normal_apply(pf)[fs.keep_cols]
            ZW, M, lab = _host_blocks(layout, bias, keep, Wk, cb, cg)
            qr, conds = _host_reduced(A, n_kept, ZW, M, lab, pc)
            sizes = sorted(sum(1 for k in lab if k == ('grid', s)) for s in range(layout[3].size))
            err = np.abs(q - qr).max() / np.abs(qr).max()
            acted = np.abs(q - q_bs).max() / np.abs(qr).max()
            print(f'{tag}: err {err:.2e} (limit 1e-12), max cond {max(conds):.2e}, blocks {sizes}, grids change q by {acted:.2e}')
            assert max(conds) <= 1e6, (tag, conds)
            if name == 'sizes':
                assert sizes == [5, 66, 67, 68]
            if name == 'cap':
                assert sizes == [64, 63 + MAX_DENSE]
            assert err <= 1e-12, (tag, err)
            if name == 'none':           # no row in any grid: the grids cannot act
                assert np.array_equal(q, q_bs), tag
            else:
                assert acted > 1e-9, (tag, acted)
            assert np.array_equal(q, fs.solver.normal_apply(pf)[fs.keep_cols]), tag   # run to run
            fs.solver.set_sensor_grids(*CLEAR)
            assert np.array_equal(q_bs, fs.solver.normal_apply(pf)[fs.keep_cols]), tag   # cleared: the bias path alone
            fs.solver.set_data_bias(None, None)
    finally:
        fs.close()


def _system(seed):
    S, fs, w, rhs = _synthetic_system('t64')
    rng = np.random.default_rng(seed)
    keep = rng.random(fs.n_data) > 0.1
    layout = _layouts(fs.n_data, keep, rng)['sizes']
    bias = _bias_part(layout[0], rng, groups=(0, 2), loose_group=True)
    cb, cg = _c(bias, w, fs.n_data)
    return fs, w, rhs, rng, keep, layout, bias, cb, cg


def test_refusals_leave_the_handle_unchanged(gpu_available):
    fs, w, rhs, rng, keep, layout, bias, cb, cg = _system(42)
    grid, node, wt, n_nodes, K = layout
    ids, nb, grp, u, ngrp = bias
    try:
        _set_bias(fs, bias, cb, cg)
        x0 = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
        it0, b0, g0 = fs.stats['iters'], fs.solver.data_bias(), fs.solver.data_slope()
        # an ID over a grid's rows and rows outside every grid
        i = int(np.flatnonzero((grid < 0) & (grp < 0))[0])
        fs.solver.set_data_bias(np.where(np.arange(ids.size) == i, 0, ids), cb)
        fs.solver.set_data_slope(grp, u, cg)
        with pytest.raises(NativeError, match='nested'):
            fs.solver.set_sensor_grids(*layout, joint=True)
        # a group likewise: group 0 lies in grid 0 and takes a row outside every grid
        fs.solver.set_data_bias(ids, cb)
        fs.solver.set_data_slope(np.where(np.arange(ids.size) == i, 0, grp), u, cg)
        with pytest.raises(NativeError, match='nested'):
            fs.solver.set_sensor_grids(*layout, joint=True)
        # a row of a grid outside its grid's group: still nested
        fs.solver.set_data_slope(np.where(np.arange(ids.size) == int(np.flatnonzero(grid == 0)[0]), -1, grp), u, cg)
        fs.solver.set_sensor_grids(*layout, joint=True)
        fs.solver.set_sensor_grids(*CLEAR)
        # 17 dense nodes in grid 0: 15 IDs and a group
        rows = np.flatnonzero(grid == 0)
        many = ids.copy()
        many[rows] = nb + np.arange(rows.size) % 15
        fs.solver.set_data_bias(many, np.full(nb + 15, cb[0]))
        fs.solver.set_data_slope(grp, u, cg)
        with pytest.raises(NativeError, match='cap'):
            fs.solver.set_sensor_grids(*layout, joint=True)
        with pytest.raises(NativeError):
            fs.solver.sensor_grids()           # none set
        # the refused calls set nothing: the same bits as before
        _set_bias(fs, bias, cb, cg)
        assert np.array_equal(fs.solve(w, keep, rhs, precond=3, method=1, **TOL), x0) and fs.stats['iters'] == it0
        assert np.array_equal(fs.solver.data_bias(), b0) and np.array_equal(fs.solver.data_slope(), g0)
        # everything lsq_set_sensor_grids refuses but the biases
        bad = node.copy()
        bad[int(np.flatnonzero(grid == 1)[0]), 2] = n_nodes[1]       # a dense node is no lattice node
        with pytest.raises(NativeError, match='node'):
            fs.solver.set_sensor_grids(grid, bad, wt, n_nodes, K, joint=True)
        with pytest.raises(NativeError, match='biases'):
            fs.solver.set_sensor_grids(*layout)                      # the plain call goes on refusing
        assert np.array_equal(fs.solve(w, keep, rhs, precond=3, method=1, **TOL), x0) and fs.stats['iters'] == it0
        fs.solver.set_sensor_grids(*layout, joint=True)
        xj = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
        itj, bj, gj, aj = fs.stats['iters'], fs.solver.data_bias(), fs.solver.data_slope(), fs.solver.sensor_grids()
        with pytest.raises(NativeError, match='sensor grids'):
            fs.solver.set_data_bias(ids, cb)
        with pytest.raises(NativeError, match='sensor grids'):
            fs.solver.set_data_slope(grp, u, cg)
        # the clearing forms too: the blocks hold the claimed IDs and groups
        with pytest.raises(NativeError, match='sensor grids'):
            fs.solver.set_data_bias(None, None)
        with pytest.raises(NativeError, match='sensor grids'):
            fs.solver.set_data_slope(None, None, None)
        assert np.array_equal(fs.solve(w, keep, rhs, precond=3, method=1, **TOL), xj) and fs.stats['iters'] == itj
        assert np.array_equal(fs.solver.data_bias(), bj) and np.array_equal(fs.solver.data_slope(), gj)
        assert np.array_equal(fs.solver.sensor_grids(), aj) and np.any(xj != x0)
        with pytest.raises(NativeError, match='CGNR'):
            fs.solve(w, keep, rhs, precond=3, method=0, **TOL)
    finally:
        fs.close()


def test_clearing_restores_every_bit_and_values_read_back(gpu_available):
    """Biases + slopes solve; joint grids set, solved (its biases, slopes and grids equal to the host's
    M⁻¹ZᵀW²(d − A_d x) for the x it returned) and cleared; then the first solve's bits again."""
    fs, w, rhs, rng, keep, layout, bias, cb, cg = _system(43)
    ids, nb, grp, u, ngrp = bias
    try:
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(np.concatenate([keep, np.ones(fs.n_con, bool)]))
        A = fs.solver.get_csr()
        _set_bias(fs, bias, cb, cg)
        x0 = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
        it0, b0, g0 = fs.stats['iters'], fs.solver.data_bias(), fs.solver.data_slope()
        for precond in (3, 1, 4):
            fs.solver.set_sensor_grids(*layout, joint=True)
            x = fs.solve(w, keep, rhs, precond=precond, method=1, **TOL)
            b, g, a = fs.solver.data_bias(), fs.solver.data_slope(), fs.solver.sensor_grids()
            assert fs.stats['method'] == 1 and fs.stats['istop'] in (1, 2), (precond, fs.stats)
            assert np.array_equal(x, fs.solve(w, keep, rhs, precond=precond, method=1, **TOL))   # run to run
            assert np.array_equal(b, fs.solver.data_bias()) and np.array_equal(a, fs.solver.sensor_grids())
            assert x.size == A.shape[1] and b.size == nb and g.shape == (ngrp, 2) and a.size == layout[3].sum()
            Wk = w[:fs.n_data][keep]
            ZW, M, lab = _host_blocks(layout, bias, keep, Wk, cb, cg)
            n_kept = int(keep.sum())
            ref = np.linalg.solve(M, ZW.T @ (Wk * rhs[:fs.n_data][keep] - (A @ x)[:n_kept]))
            got = np.concatenate([b, g.ravel(), a])
            err = np.abs(got - ref).max() / np.abs(ref).max()
            print(f'precond {precond}: {fs.stats["iters"]} iterations, read-back against the host {err:.2e}')
            assert err <= 1e-9, (precond, err)
            assert np.any(x != x0)
            fs.solver.set_sensor_grids(*CLEAR)
            with pytest.raises(NativeError):
                fs.solver.sensor_grids()
        assert np.array_equal(fs.solve(w, keep, rhs, precond=3, method=1, **TOL), x0) and fs.stats['iters'] == it0
        assert np.array_equal(fs.solver.data_bias(), b0) and np.array_equal(fs.solver.data_slope(), g0)
    finally:
        fs.close()


def test_without_biases_the_joint_call_gives_the_plain_bits(gpu_available):
    fs, w, rhs, rng, keep, layout, bias, cb, cg = _system(44)
    try:
        res = []
        for joint in (False, True):
            fs.solver.set_sensor_grids(*layout, joint=joint)
            x = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
            res.append((x, fs.stats['iters'], fs.solver.sensor_grids()))
            fs.solver.set_sensor_grids(*CLEAR)
        assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1] and np.array_equal(res[0][2], res[1][2])
    finally:
        fs.close()


def test_warm_start_after_a_mask_change(gpu_available):
    fs, w, rhs, rng, keep1, layout, bias, cb, cg = _system(45)
    ids = bias[0]
    keep2 = keep1 & (rng.random(fs.n_data) > 0.05) & (ids != 1)      # the claimed ID of grid 1 fully masked
    assert np.any(keep1[ids == 1]) and np.all(layout[0][ids == 1] == 1)
    w2 = w * np.where(np.arange(w.size) < fs.n_data, rng.uniform(0.5, 2, w.size), 1.0)
    try:
        _set_bias(fs, bias, cb, cg)
        fs.solver.set_sensor_grids(*layout, joint=True)

        def vals():
            return np.concatenate([fs.solver.data_bias(), fs.solver.data_slope().ravel(), fs.solver.sensor_grids()])

        x1 = fs.solve(w2, keep1, rhs, precond=3, method=1, **TOL)
        xw = fs.solve(w2, keep2, rhs, x0=x1, precond=3, method=1, **TOL)
        aw, it_warm = vals(), fs.stats['iters']
        xc = fs.solve(w2, keep2, rhs, precond=3, method=1, **TOL)
        ac, it_cold = vals(), fs.stats['iters']
        xj = fs.solve(w2, keep2, rhs, x0=x1, precond=1, method=1, **TOL)
    finally:
        fs.close()
    assert np.linalg.norm(xw - xc) / np.linalg.norm(xc) <= 1e-8
    assert np.linalg.norm(xj - xc) / np.linalg.norm(xc) <= 1e-8
    assert np.linalg.norm(aw - ac) / np.linalg.norm(ac) <= 1e-8
    assert it_warm < it_cold


# ---- the reference's recorded system (tests/golden/sys_sgrid_joint.npz) -----------------------------
REL, ABS = 1e-6, 1e-4                      # the tolerances of test_gpu_sgrid.py
NAMES = ['sensor_1.0_bias', 'sensor_2.0_bias', 'sensor_4.0_bias']


def _weights_rhs(S):
    w = 1. / np.concatenate((S['Ed'], S['Ec']))
    rhs = np.zeros(w.size)
    rhs[:S['data'].size] = S['data'].z
    return w, rhs


def test_eliminated_solve_reaches_the_oracle(gpu_available):
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    from lssurf_amd.smooth_fit import FitSystem
    from test_sgrid_joint_host import N_ID, N_SG, N_SLOPE, joint_objects
    g, kw, Sg, Sf, ids, c, slope = joint_objects()
    xs = g['x']
    n_grid = xs.size - N_ID - N_SLOPE - N_SG
    xb, xg, xa = np.split(xs[n_grid:], [N_ID, N_ID + N_SLOPE])
    keep = reference_epoch_keep_cols(Sg['G_data'].col_N, Sg['grids']['dz'], kw['reference_epoch'])
    assert keep.size == n_grid and xa.size == N_SG == 133
    w, rhs = _weights_rhs(Sg)
    with pytest.raises(ValueError, match='do not go together'):
        FitSystem(Sg['G_data'], Sg['Gc'], keep, Sg['Gc'].col_N, grids=Sg['grids'], bias=(ids, c, slope),
                  sensor_grids=Sf['sensor_grids'])
    ran = []
    fs = FitSystem(Sg['G_data'], Sg['Gc'], keep, Sg['Gc'].col_N, grids=Sg['grids'], bias=(ids, c, slope),
                   sensor_grids=Sf['sensor_grids'], joint=True)
    try:
        for precond in (1, 3, 4):
            ok, why = fs.solver.cg_available(precond)
            assert ok, (precond, why)
            x = fs.solve(w, np.ones(fs.n_data, bool), rhs, precond=precond, method=1, maxit=200000, **TOL)
            b, gam, a = fs.solver.data_bias(), fs.solver.data_slope().ravel(), fs.sg_vals.copy()
            assert np.array_equal(a[63:98], fs.solver.sensor_grids()[63:98] + 0.25)   # the magnitude prior of grid 2
            assert np.array_equal(a[:63], fs.solver.sensor_grids()[:63])
            ran.append(precond)
            assert fs.stats['method'] == 1 and fs.stats['istop'] in (1, 2), (precond, fs.stats)
            errs = {}
            for name, got, ref in (('grid unknowns', x, xs[:n_grid]), ('biases', b, xb), ('slopes', gam, xg),
                                   ('sensor grids', a, xa)):
                errs[name] = (np.linalg.norm(got - ref) / np.linalg.norm(ref), np.max(np.abs(got - ref)))
            print(f'precond {precond}: {fs.stats["iters"]} iterations, ' +
                  ', '.join(f'{k} {r:.2e} / {m:.2e}' for k, (r, m) in errs.items()))
            for name, (r, m) in errs.items():
                assert r <= REL and m <= ABS, (precond, name, r, m)
            # the reference's column order: z0 and dz, the biases, the slopes, the sensor grids
            assert np.array_equal(fs.expand(x)[fs.n_full:], np.concatenate([b, gam, a]))
    finally:
        fs.close()
    assert ran == [1, 3, 4], ran


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    ok = np.isfinite(b)
    return np.linalg.norm(a[ok] - b[ok]) / max(np.linalg.norm(b[ok]), 1e-300)


def _fixture_kwargs():
    from conftest import golden, golden_kwargs
    g = golden('sys_sgrid_joint.npz')
    kw = golden_kwargs(g)
    kw['data_slope_sensors'] = np.array(kw['data_slope_sensors'])
    return g, kw


@pytest.mark.parametrize('mode', ['eliminate', 'auto'])
def test_smooth_fit_runs_the_three_terms_jointly(gpu_available, mode):
    import lssurf_amd as LS
    from conftest import golden_points
    g, kw = _fixture_kwargs()
    S = LS.smooth_fit(data=golden_points(g), lsq_bias=mode, lsq_dense_max=0, lsq_sgrid_joint=True, **kw)
    d, m = S['data'], S['m']
    assert int(np.sum(d.three_sigma_edit != g['data_three_sigma_edit'].astype(bool))) == 0
    assert _rel(d.sigma_extra, g['data_sigma_extra']) < 1e-5
    assert _rel(m['z0'].z0, g['z0']) < 1e-6
    assert _rel(m['dz'].dz, g['dz']) < 1e-6
    assert _rel(d.z_est, g['data_z_est']) < 1e-6
    assert m['all'].size == g['m_all'].size and _rel(m['all'], g['m_all']) < 1e-6
    bias = m['bias']
    assert np.array_equal(bias['ID'], g['bias_ID']) and np.array_equal(bias['expected'], g['bias_expected'])
    assert np.linalg.norm(np.array(bias['val']) - g['bias_val']) <= 1e-6 * np.linalg.norm(g['bias_val'])
    assert np.array_equal(bias['N_raw'], g['bias_N_raw']) and np.array_equal(bias['N_edited'], g['bias_N_edited'])
    slope = m['slope_bias']
    assert [float(k) for k in slope] == list(g['slope_keys'])
    val = np.array([[slope[k]['slope_x'], slope[k]['slope_y']] for k in slope])
    assert np.abs(val - g['slope_val']).max() <= 1e-6 * np.linalg.norm(g['slope_val'])
    assert list(m['sensor_bias_grids']) == NAMES
    for k, name in enumerate(NAMES):
        sg = m['sensor_bias_grids'][name]
        assert np.array_equal(sg.x, g[f'sgrid{k}_x']) and np.array_equal(sg.y, g[f'sgrid{k}_y'])
        assert sg.z.shape == g[f'sgrid{k}_z'].shape and _rel(sg.z, g[f'sgrid{k}_z']) < 1e-6
    n_sg = sum(g[f'sgrid{k}_z'].size for k in range(3))
    assert np.array_equal(m['all'][-n_sg:], np.concatenate([m['sensor_bias_grids'][n].z.ravel() for n in NAMES]))
    assert np.array_equal(m['all'][-n_sg - 6:-n_sg], val.ravel())
    assert np.array_equal(m['all'][-n_sg - 6 - len(bias['val']):-n_sg - 6], bias['val'])
    t = S['timing']
    assert t['sensor_grids'] == 'eliminate' and t['sgrid_joint'] is True and t['formation'] == 'stencil'
    assert t['lsq_last']['method'] == 1


def test_smooth_fit_without_the_key_and_not_nested(gpu_available):
    import lssurf_amd as LS
    from conftest import golden_points
    g, kw = _fixture_kwargs()
    # without the key: today's refusal and today's warning
    with pytest.raises(NotImplementedError, match='bias_params'):
        LS.smooth_fit(data=golden_points(g), lsq_bias='eliminate', lsq_dense_max=0, **kw)
    with pytest.warns(RuntimeWarning, match="takes 'columns'"):
        S = LS.smooth_fit(data=golden_points(g), lsq_bias='auto', lsq_dense_max=0, **kw)
    assert S['timing']['sensor_grids'] == 'columns' and S['timing']['sgrid_joint'] is False
    assert _rel(S['m']['all'], g['m_all']) < 1e-6
    # with the key and biases per cycle, which no sensor's grid nests
    kc = {k: v for k, v in kw.items() if k != 'data_slope_sensors'}
    kc['bias_params'] = ['cycle']
    with pytest.raises(NativeError, match='nested'):
        LS.smooth_fit(data=golden_points(g), lsq_bias='eliminate', lsq_dense_max=0, lsq_sgrid_joint=True, **kc)
    with pytest.warns(RuntimeWarning, match="takes 'columns'"):
        S = LS.smooth_fit(data=golden_points(g), lsq_bias='auto', lsq_dense_max=0, lsq_sgrid_joint=True, **kc)
    assert S['timing']['sensor_grids'] == 'columns' and S['timing']['formation'] == 'coo'
    assert S['timing']['sgrid_joint'] is False and list(S['m']['sensor_bias_grids']) == NAMES


def test_profile_runs_real_iterations_over_the_joint_step(gpu_available):
    """profile_sensor_grids beside biases and slopes: real steps (the same estimates after 16 as plain
    iterations give), four positive times, and byte figures that with the bias path's own are the two
    eliminations' share of bytes_per_iter."""
    from test_gpu_cgnr import _profiler_runs_real_iterations, _times_are_positive
    fs, w, rhs, rng, keep, layout, bias, cb, cg = _system(46)

    def it(k):
        return fs.solver.iterate(rhs, k, precond=3, method=1, b_rows=fs.n_data)

    def restart():
        fs.solver.set_sensor_grids(*CLEAR)
        fs.solver.set_sensor_grids(*layout, joint=True)

    try:
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(np.concatenate([keep, np.ones(fs.n_con, bool)]))
        plain = it(1)['bytes_per_iter']
        _set_bias(fs, bias, cb, cg)
        fs.solver.set_sensor_grids(*layout, joint=True)
        prof = _profiler_runs_real_iterations(fs.solver, rhs, fs.n_data,
                                              lambda reps: fs.solver.profile_sensor_grids(reps=reps), restart)
        assert list(prof) == ['btd', 'trsv_t', 'trsv', 'apply']
        _times_are_positive([ms for ms, _ in prof.values()])
        joint = it(1)['bytes_per_iter']
        bias_bytes = sum(b for _, b in fs.solver.profile_data_slope(reps=1).values())
        assert sum(b for _, b in prof.values()) + bias_bytes == joint - plain
    finally:
        fs.close()
