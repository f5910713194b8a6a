"""Slope biases eliminated inside CGNR with the data biases (lsq_set_data_slope; csrc/slope.inc) and
smooth_fit's data_slope_sensors.

Operator: lsq_normal_apply with slopes set must equal AᵀA p − A_dᵀ W Z M⁻¹ Zᵀ W A_d p with Z = [B U] and
M = ZᵀW²Z + C² formed densely on the host from the assembled A, to the normal operator's own tolerance,
1e-12 of max|q|, on the layouts that can break a segmented sum or the per-group reduction, each with
biases and without (nb = 0).  The host asserts cond(G_s) ≤ 1e3 there, so the tolerance means
something; the collinear layout's limit is 10 × the error of the host's own float64 Schur form
against an extended-precision dense solve (or 1e-12 if that is larger).  Solves: the reference's
recorded system (tests/golden/sys_slope.npz, gen_golden_slope.py) within REL 1e-6 / ABS 1e-4;
smooth_fit against the reference's outputs with the tolerances of test_gpu_bias.py."""
import functools

import numpy as np
import pytest

import lssurf_amd as LS
from conftest import golden, golden_kwargs, golden_points
from lssurf_amd._native import NativeError
from lssurf_amd.bias_functions import assign_bias_ID
from lssurf_amd.constraint_functions import reference_epoch_keep_cols
from lssurf_amd.data_slope_bias import slope_columns
from lssurf_amd.smooth_fit import FitSystem
from test_gpu_cgnr import _profiler_runs_real_iterations, _synthetic_system, _times_are_positive

pytestmark = pytest.mark.gpu
REL, ABS = 1e-6, 1e-4
TOL = dict(atol=1e-12, btol=1e-12, conlim=1e12)
PARAMS = ['sensor', 'cycle']
GROUP_SIZES = [1, 63, 64, 65, 511, 512, 513]
IDS_PER_GROUP = [1, 63, 64, 65, 130]
LONG_GROUP = 32 * 512 + 300   # rows of a group whose ranks span more than 32 chunks wherever they start


def _ids_nested(grp, ng, per_group, n_free, rng):
    """Bias IDs that nest in the groups: per_group[g] IDs for the rows of group g (every ID gets a
    row when the group has enough), n_free IDs for the rows outside every group."""
    ids = np.empty(grp.size, np.int32)
    first = 0
    for g in range(ng):
        rows = np.flatnonzero(grp == g)
        k = per_group[g]
        mine = rng.integers(0, k, rows.size)
        mine[:min(k, rows.size)] = np.arange(min(k, rows.size))
        ids[rows] = first + mine
        first += k
    out = grp < 0
    ids[out] = first + rng.integers(0, n_free, int(out.sum()))
    return ids, first + n_free


def _deal(npts, sizes, rng):
    grp = np.full(npts, -1, np.int32)
    order = rng.permutation(npts)
    k = 0
    for g, n in enumerate(sizes):
        grp[order[k:k + n]] = g
        k += n
    return grp


def _layouts(npts, keep, rng):
    """name -> (ids, c, grp, u, cs)"""
    out = {}
    u = rng.standard_normal((npts, 2))

    def add(name, grp, ng, per_group, n_free=3, u=u):
        ids, nb = _ids_nested(grp, ng, per_group, n_free, rng)
        out[name] = (ids, rng.uniform(1., 30., nb), grp, u, rng.uniform(1., 5., (ng, 2)))

    # groups of the critical sizes dealt out by a random permutation of the points, so no group is
    # contiguous in the solver's cell-sorted order; the ID of the one-row group also holds rows outside
    grp = _deal(npts, GROUP_SIZES, rng)
    add('sizes', grp, len(GROUP_SIZES), [1, 2, 1, 3, 2, 1, 4])
    ids = out['sizes'][0]
    ids[np.flatnonzero(grp < 0)[:40]] = 0
    # a group all of whose rows are masked: the masked rows are group 0
    add('masked_group', np.where(keep, 1 + rng.integers(0, 3, npts), 0).astype(np.int32), 4, [2, 2, 2, 2])
    # a group in [0, ng) that no row carries
    g_e = rng.integers(-1, 4, npts).astype(np.int32)
    g_e[g_e == 2] = 3
    add('empty_group', g_e, 4, [2, 2, 2, 2])
    # every row outside the groups
    add('none', np.full(npts, -1, np.int32), 2, [1, 1])
    # groups that hold 1, 63, 64, 65 and 130 bias IDs (about 8 rows each)
    add('many_ids', _deal(npts, [8 * k for k in IDS_PER_GROUP], rng), len(IDS_PER_GROUP), IDS_PER_GROUP)
    # a collinear group: u₁ = 2 u₀ on its rows, so F has rank one and G is ill-conditioned
    g_c = _deal(npts, [700, 300], rng)
    u_c = u.copy()
    u_c[g_c == 0, 1] = 2 * u_c[g_c == 0, 0]
    add('collinear', g_c, 2, [2, 1], u=u_c)
    if npts >= 2 * LONG_GROUP + 2000:
        # a group (and, with biases, a rank in it) over more than 32 chunks, beside a long rank outside
        # every group and short ones
        add('long', _deal(npts, [LONG_GROUP, 700, 65], rng), 3, [1, 2, 1], n_free=1)
    return out


def _dense_Z(idk, c, grpk, uk, cs):
    """Z = [B U] on the kept rows and the diagonal of C²."""
    n, nb, ng = idk.size if idk is not None else grpk.size, (c.size if c is not None else 0), cs.shape[0]
    Z = np.zeros((n, nb + 2 * ng))
    if nb:
        Z[np.arange(n), idk] = 1.0
    on = grpk >= 0
    Z[on, nb + 2 * grpk[on]] = uk[on, 0]
    Z[on, nb + 2 * grpk[on] + 1] = uk[on, 1]
    C2 = np.concatenate([c ** 2 if nb else np.zeros(0), cs.ravel() ** 2])
    return Z, C2


def _chol_solve_ld(M, r):
    """M⁻¹ r in extended precision (plain Cholesky; M small, symmetric positive definite)."""
    n = M.shape[0]
    L = np.zeros((n, n), np.longdouble)
    for j in range(n):
        L[j, j] = np.sqrt(M[j, j] - L[j, :j] @ L[j, :j])
        for i in range(j + 1, n):
            L[i, j] = (M[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n, np.longdouble)
    for i in range(n):
        y[i] = (r[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, np.longdouble)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def _host_reduced(A, n_kept, Wk, idk, c, grpk, uk, cs, pc, extended=False):
    """((AᵀA − A_dᵀ W Z M⁻¹ Zᵀ W A_d) p, the groups' cond(G_s)) from the assembled, weighted,
    row-selected A (data rows first) with Z and M dense."""
    Ad = A[:n_kept]
    t = Ad @ pc                                               # W A_d p
    Z, C2 = _dense_Z(idk, c, grpk, uk, cs)
    nb, ng = Z.shape[1] - 2 * cs.shape[0], cs.shape[0]
    ZW = Wk[:, None] * Z
    if extended:
        ZWl = ZW.astype(np.longdouble)
        M = ZWl.T @ ZWl + np.diag(C2.astype(np.longdouble))
        sol = _chol_solve_ld(M, ZWl.T @ t.astype(np.longdouble)).astype(float)
    else:
        M = ZW.T @ ZW + np.diag(C2)
        sol = np.linalg.solve(M, ZW.T @ t)
    M = np.asarray(M, float)
    G = M[nb:, nb:] - (M[nb:, :nb] @ np.linalg.solve(M[:nb, :nb], M[:nb, nb:]) if nb else 0.0)
    conds = [np.linalg.cond(G[2 * s:2 * s + 2, 2 * s:2 * s + 2]) for s in range(ng)]
    off = G.copy()
    for s in range(ng):
        off[2 * s:2 * s + 2, 2 * s:2 * s + 2] = 0
    assert np.abs(off).max() <= 1e-9 * np.abs(G).max()      # nested: one 2 × 2 block per group
    return A.T @ (A @ pc) - Ad.T @ (ZW @ sol), conds


def _host_schur64(A, n_kept, Wk, idk, c, grpk, uk, cs, pc):
    """The same operator by the device's formulas in float64 (per-ID and per-group sums, one 2 × 2
    Cholesky per group): the error a float64 Schur form has of its own."""
    Ad = A[:n_kept]
    t = Wk * (Ad @ pc)                                        # td = W² A_d p
    ng = cs.shape[0]
    on = grpk >= 0
    w2 = Wk ** 2
    gam = np.zeros((ng, 2))
    if c is not None:
        nb = c.size
        sg = np.full(nb, -1)
        sg[idk[on]] = grpk[on]
        D = np.bincount(idk, weights=w2, minlength=nb) + c ** 2
        s = np.bincount(idk, weights=t, minlength=nb)
        e = np.stack([np.bincount(idk, weights=w2 * np.where(on, uk[:, k], 0), minlength=nb) for k in (0, 1)], 1)
    for g in range(ng):
        r = grpk == g
        F = (uk[r] * w2[r, None]).T @ uk[r] + np.diag(cs[g] ** 2)
        h = uk[r].T @ t[r]
        if c is not None:
            j = sg == g
            F = F - (e[j] / D[j, None]).T @ e[j]
            h = h - e[j].T @ (s[j] / D[j])
        L = np.linalg.cholesky(F)
        gam[g] = np.linalg.solve(L.T, np.linalg.solve(L, h))
    corr = np.where(on, np.sum(uk * gam[np.where(on, grpk, 0)], axis=1), 0.0)
    if c is not None:
        beta = (s - np.where(sg >= 0, np.sum(e * gam[np.where(sg >= 0, sg, 0)], axis=1), 0.0)) / D
        corr = corr + beta[idk]
    return A.T @ (A @ pc) - Ad.T @ (Wk * corr)


@pytest.mark.parametrize('which', ['t64', 'tdense'])
def test_reduced_normal_operator(gpu_available, which):
    S, fs, w, rhs = _synthetic_system(which)
    rng = np.random.default_rng(21)
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
        q_plain = fs.solver.normal_apply(pf)[fs.keep_cols]
        layouts = _layouts(fs.n_data, keep, rng)
        assert ('long' in layouts) == (which == 'tdense')
        if which == 'tdense':            # the small system runs the others
            layouts = {k: layouts[k] for k in ('long', 'sizes')}
        for name, (ids, c, grp, u, cs) in layouts.items():
            for with_bias in (True, False):
                tag = f'{which} {name} {"biases" if with_bias else "nb=0"}'
                if with_bias:
                    fs.solver.set_data_bias(ids, c)
                    q_base = fs.solver.normal_apply(pf)[fs.keep_cols]
                else:
                    fs.solver.set_data_bias(None, None)
                    q_base = q_plain
                fs.solver.set_data_slope(grp, u, cs)
                ok, why = fs.solver.cg_available(1)
                assert ok, (tag, why)
                q = fs.solver.normal_apply(pf)[fs.keep_cols]
                host = (A, n_kept, Wk, ids[keep] if with_bias else None, c if with_bias else None, grp[keep], u[keep],
                        cs, pc)
                if name == 'collinear':
                    qr, conds = _host_reduced(*host, extended=True)
                    own = np.abs(_host_schur64(*host) - qr).max() / np.abs(qr).max()
                    limit = max(10 * own, 1e-12)
                    assert max(conds) > 1e3, (tag, conds)
                else:
                    qr, conds = _host_reduced(*host)
                    own, limit = 0.0, 1e-12
                    assert max(conds) <= 1e3, (tag, conds)
                err = np.abs(q - qr).max() / np.abs(qr).max()
                acted = np.abs(q - q_base).max() / np.abs(qr).max()
                print(f'{tag}: err {err:.2e} (limit {limit:.2e}, host float64 Schur {own:.2e}), max cond(G) '
                      f'{max(conds):.2e}, slopes change q by {acted:.2e}')
                assert err <= limit, (tag, err, limit)
                if name == 'none':       # no row in any group: the slopes cannot act
                    assert acted <= 1e-12, (tag, acted)
                else:
                    assert acted > 1e-9, (tag, acted)
                assert np.array_equal(q, fs.solver.normal_apply(pf)[fs.keep_cols]), tag   # run to run
    finally:
        fs.close()


def test_a_layout_that_is_not_nested_is_refused(gpu_available):
    S, fs, w, rhs = _synthetic_system('t64')
    rng = np.random.default_rng(22)
    keep = rng.random(fs.n_data) > 0.1
    ids, c, grp, u, cs = _layouts(fs.n_data, keep, rng)['sizes']
    try:
        fs.solver.set_data_bias(ids, c)
        x0 = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
        b0, it0 = fs.solver.data_bias(), fs.stats['iters']
        bad = grp.copy()
        rows = np.flatnonzero(ids == ids[np.flatnonzero(grp == 4)[0]])   # one ID's rows …
        bad[rows[0]] = 5                                                  # … in two groups
        with pytest.raises(NativeError, match='nested'):
            fs.solver.set_data_slope(bad, u, cs)
        with pytest.raises(NativeError, match='outside'):
            fs.solver.set_data_slope(np.where(np.arange(grp.size) == 3, len(cs), grp), u, cs)
        with pytest.raises(NativeError, match='outside'):
            fs.solver.set_data_slope(np.where(np.arange(grp.size) == 3, -2, grp), u, cs)
        ub = u.copy()
        ub[np.flatnonzero(grp >= 0)[0], 1] = np.nan
        with pytest.raises(NativeError, match='finite'):
            fs.solver.set_data_slope(grp, ub, cs)
        for v in (0.0, -1.0, np.nan):
            cb = cs.copy()
            cb[2, 1] = v
            with pytest.raises(NativeError, match='> 0'):
                fs.solver.set_data_slope(grp, u, cb)
        with pytest.raises(NativeError, match='npts'):
            fs.solver.set_data_slope(grp[:-1], u[:-1], cs)
        with pytest.raises(NativeError):
            fs.solver.data_slope()         # none set
        # the refused calls set nothing: the same bits as before
        assert np.array_equal(fs.solve(w, keep, rhs, precond=3, method=1, **TOL), x0)
        assert np.array_equal(fs.solver.data_bias(), b0) and fs.stats['iters'] == it0
        # a NaN outside every group is never read
        un = u.copy()
        un[grp < 0] = np.nan
        fs.solver.set_data_slope(grp, un, cs)
        with pytest.raises(NativeError, match='no lsq_solve'):
            fs.solver.data_slope()         # set, not solved
        with pytest.raises(NativeError, match='CGNR'):
            fs.solve(w, keep, rhs, precond=3, method=0, **TOL)
        xs = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
        assert np.all(np.isfinite(xs)) and np.any(xs != x0) and np.any(fs.solver.data_slope() != 0)
    finally:
        fs.close()


def test_clearing_the_slopes_restores_every_bit(gpu_available):
    res = []
    for with_slope in (False, True):
        S, fs, w, rhs = _synthetic_system('t64')
        keep = np.random.default_rng(24).random(fs.n_data) > 0.1
        ids, c, grp, u, cs = _layouts(fs.n_data, keep, np.random.default_rng(25))['sizes']
        try:
            fs.solver.set_data_bias(ids, c)
            if with_slope:
                fs.solver.set_data_slope(grp, u, cs)
                xs = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
                assert np.array_equal(xs, fs.solve(w, keep, rhs, precond=3, method=1, **TOL))   # run to run
                fs.solver.set_data_slope(None, None, None)
                with pytest.raises(NativeError):
                    fs.solver.data_slope()
            x = fs.solve(w, keep, rhs, precond=3, method=1, **TOL)
            res.append((x, fs.solver.data_bias(), fs.stats['iters']))
        finally:
            fs.close()
    assert np.any(xs != res[1][0])
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2]


def test_profile_data_slope_runs_real_iterations(gpu_available):
    """profile_data_slope: refused without the live state of iterate() and without slopes (the handle
    goes on iterating); on the live state it runs real steps (the same estimates after 16 as plain
    iterations give), its four times are positive, and its four byte figures are the elimination's
    share of bytes_per_iter."""
    S, fs, w, rhs = _synthetic_system('t64')
    keep = np.random.default_rng(26).random(fs.n_data) > 0.1
    ids, c, grp, u, cs = _layouts(fs.n_data, keep, np.random.default_rng(27))['sizes']

    def it(k):
        return fs.solver.iterate(rhs, k, precond=3, method=1, b_rows=fs.n_data)

    try:
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(np.concatenate([keep, np.ones(fs.n_con, bool)]))
        fs.solver.set_data_bias(ids, c)
        fs.solver.set_data_slope(grp, u, cs)
        with pytest.raises(NativeError, match='live state'):
            fs.solver.profile_data_slope(reps=3)
        prof = _profiler_runs_real_iterations(fs.solver, rhs, fs.n_data,
                                              lambda reps: fs.solver.profile_data_slope(reps=reps),
                                              lambda: fs.solver.set_data_slope(grp, u, cs))
        assert list(prof) == ['chunk', 'rank', 'group', 'apply']
        _times_are_positive([ms for ms, _ in prof.values()])
        with_slopes = it(1)['bytes_per_iter']
        fs.solver.set_data_bias(None, None)          # the biases and the slopes
        without = it(1)
        assert sum(b for _, b in prof.values()) == with_slopes - without['bytes_per_iter']
        with pytest.raises(NativeError, match='no slopes'):
            fs.solver.profile_data_slope(reps=3)      # a live state, no slopes
        assert it(2)['iters'] == without['iters'] + 2
    finally:
        fs.close()


@functools.lru_cache(maxsize=None)
def _slope_objects():
    """Host objects of the reference's recorded slope system: the grid-only operators, the full
    ones, IDs and c, the slope groups, coefficients and c."""
    g = golden('sys_slope.npz')
    kw = golden_kwargs(g)
    kw['data_slope_sensors'] = np.array(kw['data_slope_sensors'])
    kw_grid = {k: v for k, v in kw.items() if not k.startswith('bias_') and k != 'data_slope_sensors'}
    Sg = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, **kw_grid)
    Sf = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, lsq_bias='columns', **kw)
    D, bm = assign_bias_ID(golden_points(g), PARAMS)
    expected = np.array([bm['E_bias'][j] for j in range(len(bm['E_bias']))])
    present, grp, u = slope_columns(D, kw['data_slope_sensors'])
    assert list(present) == list(g['slope_keys'])
    cs = np.full((len(present), 2), 1. / (0.01 * 1000))
    return g, kw, Sg, Sf, D.bias_ID.astype(np.int32), 1. / expected, (grp, u, cs)


def _weights_rhs(S):
    w = 1. / np.concatenate((S['Ed'], S['Ec']))
    rhs = np.zeros(w.size)
    rhs[:S['data'].size] = S['data'].z
    return w, rhs


def test_eliminated_solve_reaches_the_oracle(gpu_available):
    g, kw, Sg, Sf, ids, c, slope = _slope_objects()
    xs = g['x']
    n_slope = slope[2].size
    n_grid = xs.size - c.size - n_slope
    xb, xg = xs[n_grid:n_grid + c.size], xs[n_grid + c.size:]
    keep = reference_epoch_keep_cols(Sg['G_data'].col_N, Sg['grids']['dz'], kw['reference_epoch'])
    assert keep.size == n_grid
    w, rhs = _weights_rhs(Sg)
    ran = []
    fs = FitSystem(Sg['G_data'], Sg['Gc'], keep, Sg['Gc'].col_N, grids=Sg['grids'], bias=(ids, c, slope))
    try:
        for precond in (1, 3, 4):
            if not fs.solver.cg_available(precond)[0]:
                continue
            x = fs.solve(w, np.ones(fs.n_data, bool), rhs, precond=precond, method=1, maxit=200000, **TOL)
            b, gam = fs.solver.data_bias(), fs.solver.data_slope().ravel()
            ran.append(precond)
            assert fs.stats['method'] == 1 and fs.stats['istop'] in (1, 2), (precond, fs.stats)
            eg = np.linalg.norm(x - xs[:n_grid]) / np.linalg.norm(xs[:n_grid])
            eb = np.linalg.norm(b - xb) / np.linalg.norm(xb)
            es = np.linalg.norm(gam - xg) / np.linalg.norm(xg)
            print(f'precond {precond}: {fs.stats["iters"]} iterations, grid {eg:.2e}, biases {eb:.2e}, slopes {es:.2e}')
            assert eg <= REL and np.max(np.abs(x - xs[:n_grid])) <= ABS, (precond, eg)
            assert eb <= 1e-6, (precond, eb)
            assert es <= 1e-6, (precond, es)
            x_el = np.concatenate([x, b, gam])
            assert np.array_equal(fs.expand(x)[fs.n_full:], np.concatenate([b, gam]))
    finally:
        fs.close()
    assert 1 in ran and 3 in ran, ran
    # the in-project cross-check: biases and slopes as ordinary columns, dense preconditioner
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
    rng = np.random.default_rng(26)
    keep1 = rng.random(fs.n_data) > 0.1
    keep2 = keep1 & (rng.random(fs.n_data) > 0.05)
    ids, c, grp, u, cs = _layouts(fs.n_data, keep1, rng)['sizes']
    w2 = w * np.where(np.arange(w.size) < fs.n_data, rng.uniform(0.5, 2, w.size), 1.0)
    try:
        fs.solver.set_data_bias(ids, c)
        fs.solver.set_data_slope(grp, u, cs)
        x1 = fs.solve(w2, keep1, rhs, precond=3, method=1, **TOL)
        xw = fs.solve(w2, keep2, rhs, x0=x1, precond=3, method=1, **TOL)
        bw, gw, it_warm = fs.solver.data_bias(), fs.solver.data_slope(), fs.stats['iters']
        xc = fs.solve(w2, keep2, rhs, precond=3, method=1, **TOL)
        bc, gc, it_cold = fs.solver.data_bias(), fs.solver.data_slope(), fs.stats['iters']
        xj = fs.solve(w2, keep2, rhs, x0=x1, precond=1, method=1, **TOL)
    finally:
        fs.close()
    assert np.linalg.norm(xw - xc) / np.linalg.norm(xc) <= 1e-8
    assert np.linalg.norm(xj - xc) / np.linalg.norm(xc) <= 1e-8
    assert np.linalg.norm(bw - bc) / np.linalg.norm(bc) <= 1e-8
    assert np.linalg.norm(gw - gc) / np.linalg.norm(gc) <= 1e-8
    assert it_warm < it_cold


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    ok = np.isfinite(b)
    return np.linalg.norm(a[ok] - b[ok]) / max(np.linalg.norm(b[ok]), 1e-300)


def _check_fit_against_reference(S, g):
    """The checks of test_gpu_bias.py's _check_fit_against_reference, with the biases' place in
    m['all'] moved in front of the slopes, and the slopes' own."""
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
    pd = S['bias_model']['bias_param_dict']
    assert pd['ID'] == [int(j) for j in g['bias_ID']]
    assert not np.any(pd.get('edited', False)) and not g['bias_edited'].any()
    assert 'constraint_data_bias' in S['TOC']['rows'] and 'constraint_data_slope' in S['TOC']['rows']
    slope = m['slope_bias']
    assert [float(k) for k in slope] == list(g['slope_keys'])
    val = np.array([[slope[k]['slope_x'], slope[k]['slope_y']] for k in slope])
    assert np.abs(val - g['slope_val']).max() <= 1e-6 * np.linalg.norm(g['slope_val'])
    assert m['all'].size == g['m_all'].size
    assert np.array_equal(m['all'][-4:], val.ravel())                       # the model ends with the 4 slopes
    assert np.array_equal(m['all'][-4 - len(bias['val']):-4], bias['val'])  # behind the biases


@pytest.mark.parametrize('mode', ['eliminate', 'columns'])
def test_smooth_fit_with_slopes_matches_reference(gpu_available, mode):
    g = golden('sys_slope.npz')
    kw = golden_kwargs(g)
    kw['data_slope_sensors'] = np.array(kw['data_slope_sensors'])
    extra = dict(lsq_bias='eliminate', lsq_dense_max=0) if mode == 'eliminate' else dict(lsq_bias='columns')
    S = LS.smooth_fit(data=golden_points(g), **kw, **extra)
    _check_fit_against_reference(S, g)
    assert S['timing']['lsq_last']['method'] == (1 if mode == 'eliminate' else 0)


def test_auto_takes_columns_where_the_layout_is_not_nested(gpu_available):
    """Biases by cycle alone: a cycle's rows lie in both slope sensors, which the device refuses;
    'eliminate' raises its reason, 'auto' runs the fit with the slopes as columns."""
    g = golden('sys_slope.npz')
    kw = golden_kwargs(g)
    kw.update(data_slope_sensors=np.array(kw['data_slope_sensors']), bias_params=['cycle'], lsq_dense_max=0)
    with pytest.raises(NativeError, match='nested'):
        LS.smooth_fit(data=golden_points(g), lsq_bias='eliminate', **kw)
    Sa = LS.smooth_fit(data=golden_points(g), lsq_bias='auto', **kw)
    Sc = LS.smooth_fit(data=golden_points(g), lsq_bias='columns', **kw)
    assert Sa['timing']['formation'] == 'coo' and Sa['timing']['lsq_last']['method'] == 0
    assert list(Sa['m']['slope_bias']) == [1., 2.]
    assert np.array_equal(Sa['m']['all'], Sc['m']['all'])
