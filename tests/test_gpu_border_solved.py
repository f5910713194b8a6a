"""GPU parity of the border term of compute_E at window scale: lsq_cov_border_solved
(lssurf_amd/csrc/bsolve.inc) and smooth_fit(lsq_E_border=True, lsq_E_border_solve=True).

The shared systems are tests/test_gpu_border.py's 17 × 17 × 6 recipe (1 734 grid columns = 27.09 panels
of 64 rows, 10 % of the data rows masked) with borders of 1, 5, 65 (one column past a panel) and the
mixed 130 biases + 2 × 2 slope columns.  The code under test runs on the GRID-ONLY structured system
(the same smooth_fit call without bias_params) with the border passed as errors.split_border makes it;
the references are cov_band_bordered on the combined system and the host float64 inverse of its
get_csr() — neither is the code under test.  The solves run CGNR + block-Jacobi at atol = btol = 1e-12.

SIGMA_TOL: ten times the largest relative σ deviation from cov_band_bordered measured over these
cases (profiles/border_solved.json, "tests"), to cover run-to-run differences of the CG path between
boxes; it must stay below 1e-5, the amount by which the reference's own R⁻¹ truncation moves σ."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import lssurf_amd as LS
from conftest import golden, golden_kwargs, golden_points
from lssurf_amd._native import NativeError, NativeRefused
from lssurf_amd.errors import band_order, bordered_band_order, split_border, window_cov
from test_gpu_border import NT, S_NODES, _build, _op_rows, _rel, _slope_kwargs

pytestmark = pytest.mark.gpu

TOL = 1e-12                 # the solves' atol and btol: the project's solve tolerance
SIGMA_TOL = 2.71e-7         # 10 × 2.71e-8 (k = 1, grid columns: the smallest pivot, 7.7e-5); see the module docstring
CASES = [1, 5, 65, 'mixed']
SOLVE = dict(atol=TOL, btol=TOL, conlim=1e12, precond=3)


def _grid_only(out, S, nt):
    """The structured grid-only fit objects of a system built by the recipe: the same call without
    bias_params (the points in the same order)."""
    from lssurf_amd import synthetic
    W = {'x': (S - 1) * 100., 'y': (S - 1) * 100., 't': (nt - 1) * 0.25}
    return LS.smooth_fit(data=out['data'], W=W, ctr={'x': 0., 'y': 0., 't': 0.},
                         spacing={'z0': 100., 'dz': 100., 'dt': 0.25}, E_RMS=dict(synthetic.E_RMS_NOTEBOOK),
                         reference_epoch=nt // 2, return_fit_objects=True)


def _build33(k):
    """test_gpu_border._build's recipe on a 33 × 33 × 4 grid"""
    from lssurf_amd import synthetic
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    from lssurf_amd.smooth_fit import FitSystem
    S, nt = 33, 4
    W = {'x': (S - 1) * 100., 'y': (S - 1) * 100., 't': (nt - 1) * 0.25}
    rng = np.random.default_rng(7)
    npts = 2 * S * S
    x, y = (rng.random(npts) - 0.5) * W['x'], (rng.random(npts) - 0.5) * W['y']
    t = (rng.random(npts) - 0.5) * W['t']
    z = 10 * np.sin(2 * np.pi * x / (W['x'] / 2)) + rng.normal(0, 0.1, npts)
    fields = {'x': x, 'y': y, 'time': t, 'z': z, 'sigma': np.full(npts, 0.1), 'sigma_corr': np.full(npts, 0.5),
              'cycle': (rng.permutation(npts) % k).astype(float)}
    out = LS.smooth_fit(data=LS.containers.data().from_dict(fields), W=W, ctr={'x': 0., 'y': 0., 't': 0.},
                        spacing={'z0': 100., 'dz': 100., 'dt': 0.25}, E_RMS=dict(synthetic.E_RMS_NOTEBOOK),
                        reference_epoch=nt // 2, return_fit_objects=True, lsq_bias='columns', bias_params=['cycle'])
    keep_cols = reference_epoch_keep_cols(out['G_data'].col_N, out['grids']['dz'], nt // 2)
    fs = FitSystem(out['G_data'], out['Gc'], keep_cols, out['Gc'].col_N)
    w = 1. / np.concatenate((out['Ed'], out['Ec']))
    keep = np.random.default_rng(3).random(fs.n_data) > 0.1
    mask = np.concatenate([keep, np.ones(fs.n_con, bool)])
    perm, n_border = bordered_band_order(out['grids'], keep_cols, int(out['grids']['dz'].col_N))
    assert n_border == k
    return out, fs, w, mask, perm, n_border


class _Pair:
    """The combined system (the references) and the grid-only system with its split border."""

    def __init__(self, built, S, nt):
        from lssurf_amd.constraint_functions import reference_epoch_keep_cols
        from lssurf_amd.smooth_fit import FitSystem
        self.out, self.full, self.w, self.mask, self.perm, self.k = built
        out = self.out
        self.n_grid = int(out['grids']['dz'].col_N)
        keep_cols = reference_epoch_keep_cols(out['G_data'].col_N, out['grids']['dz'], nt // 2)
        self.keep_g = keep_cols[keep_cols < self.n_grid]
        self.n_g = self.keep_g.size
        Sg = _grid_only(out, S, nt)
        self.grids = Sg['grids']
        G_grid, Gc_grid, self.B, self.c_con = split_border(out['G_data'], out['Gc'], out['Ec'], keep_cols, self.n_grid,
                                                           grid_ops=(Sg['G_data'], Sg['Gc']))
        try:
            self.grid = FitSystem(G_grid, Gc_grid, self.keep_g, self.n_grid, grids=self.grids)
        except Exception:
            self.full.close()
            raise
        assert self.grid.formation == 'stencil' and self.grid.has_blocks
        self.n_rows = self.grid.n_data + self.grid.n_con
        self.order_g = band_order(self.grids, self.keep_g)
        self.weigh(1.0)

    def weigh(self, f):
        for fs, n in ((self.full, self.w.size), (self.grid, self.n_rows)):
            fs.solver.set_row_weight(np.ascontiguousarray(self.w[:n] * f))
            fs.solver.set_row_mask(self.mask[:n])

    def close(self):
        self.full.close()
        self.grid.close()


@functools.lru_cache(maxsize=None)
def _case(k):
    """every device result of one border size and the host inverse, computed once"""
    P = _Pair(_build(k), S_NODES, NT)
    r = {'k': P.k, 'n_g': P.n_g}
    try:
        assert P.n_g == S_NODES * S_NODES * NT
        r['E_ref'], _, _ = P.full.solver.cov_band_bordered(P.perm, P.k)
        A = P.full.solver.get_csr()
        Ew, _, _ = P.grid.solver.cov_band_window(P.order_g)      # one window over the whole grid
        r['E_win'] = np.zeros(P.n_g)
        r['E_win'][P.order_g] = Ew
        r['va'], r['vb'], _, r['info'] = P.grid.solver.cov_border_solved(P.B, P.c_con, **SOLVE)
        r['va2'], r['vb2'], _, r['info2'] = P.grid.solver.cov_border_solved(P.B, P.c_con, **SOLVE)
        P.weigh(1.5)
        r['va_rw'], r['vb_rw'], _, _ = P.grid.solver.cov_border_solved(P.B, P.c_con * 1.5 ** 2, **SOLVE)
    finally:
        P.close()
    r['E_host'] = np.sqrt(np.diag(np.linalg.inv((A.T @ A).toarray())))
    return r


@pytest.mark.parametrize('k', CASES)
def test_whole_grid_window_plus_border_matches_both_references(gpu_available, k):
    r = _case(k)
    n_g = r['n_g']
    E = np.concatenate((np.sqrt(r['E_win'] ** 2 + r['va']), np.sqrt(r['vb'])))
    info = r['info']
    print(f"k={k}: {info['iters']} iterations (most {info['iters_max']}), solves {info['solve_us'] * 1e-6:.2f} s, "
          f"asym {info['asym']:.2e}, smallest pivot {info['min_pivot']:.3f}")
    for name, sel in (('grid', slice(0, n_g)), ('border', slice(n_g, None))):
        band, host = _rel(E[sel], r['E_ref'][sel]), _rel(E[sel], r['E_host'][sel])
        print(f'k={k} {name}: vs cov_band_bordered {band:.2e}, vs host inverse {host:.2e}')
        assert band <= SIGMA_TOL, (k, name, band)
        # the host inverse itself sits within 1e-9 of the band path (tests/test_gpu_border.py)
        assert host <= SIGMA_TOL + 1e-9, (k, name, host)
    # the border acts: without var_add the grid σ is off by more than 1e-3 (tests/test_gpu_border.py)
    assert _rel(r['E_win'], r['E_ref'][:n_g]) > 1e-3
    assert info['k_pad'] == -(-r['k'] // 64) * 64 and info['bytes'] == (1792 * info['k_pad'] + 3 * info['k_pad'] ** 2) * 8
    assert info['iters'] >= info['iters_max'] > 0 and 0 < info['min_pivot'] <= 1 and info['asym'] >= 0
    assert info['asym'] / info['min_pivot'] <= SIGMA_TOL


@pytest.mark.parametrize('k', CASES)
def test_repeats_bit_for_bit_and_reweights(gpu_available, k):
    r = _case(k)
    assert np.array_equal(r['va'], r['va2']) and np.array_equal(r['vb'], r['vb2'])
    assert r['info']['iters'] == r['info2']['iters'] and r['info']['asym'] == r['info2']['asym']
    # weights × 1.5 (c_con, already weighted, × 1.5²): every variance / 1.5².  Each run's σ lies within
    # SIGMA_TOL of the reference, so each variance within 2 SIGMA_TOL σ² and their difference within 4
    E_rw = np.concatenate((np.sqrt((r['E_win'] / 1.5) ** 2 + r['va_rw']), np.sqrt(r['vb_rw'])))
    d = _rel(E_rw * 1.5, r['E_ref'])
    print(f'k={k}: re-weighted σ vs cov_band_bordered / 1.5: {d:.2e}')
    assert d <= SIGMA_TOL, (k, d)
    n_g = r['n_g']
    for a, b, E in ((r['va_rw'], r['va'], r['E_ref'][:n_g]), (r['vb_rw'], r['vb'], r['E_ref'][n_g:])):
        d = np.abs(a * 1.5 ** 2 - b).max() / (E ** 2).max()
        print(f'k={k}: re-weighted variance off by {d:.2e} of σ²')
        assert d <= 4 * SIGMA_TOL, (k, d)


def test_several_windows_see_var_add_alone(gpu_available):
    """33 × 33 × 4, k = 5: var_add against E_bordered² − E_cov_band(grid only)², relative to E² (twice the
    relative σ bound).  The windows (tile 8, margin 6) are approximate on their own; their σ is a
    conditional variance and stays at or below the exact grid-only one."""
    P = _Pair(_build33(5), 33, 4)
    try:
        assert P.n_g == 33 * 33 * 4
        E_ref, _, _ = P.full.solver.cov_band_bordered(P.perm, P.k)
        E_grid, _, _ = P.grid.solver.cov_band(P.order_g)
        va, vb, _, info = P.grid.solver.cov_border_solved(P.B, P.c_con, **SOLVE)
        E_w, _, check = window_cov(P.grid.solver, P.grids, P.keep_g, tile=8, margin=6)
        P.grid.solver.solve(np.zeros(P.n_rows), precond=3, method=1)        # the handle still solves
    finally:
        P.close()
    ref = E_ref[:P.n_g] ** 2 - E_grid ** 2
    d = np.abs(va - ref).max() / (E_ref[:P.n_g] ** 2).max()
    db = _rel(np.sqrt(vb), E_ref[P.n_g:])
    dw = _rel(np.sqrt(E_w ** 2 + va), E_ref[:P.n_g])
    print(f'33x33x4: var_add vs E_bordered² − E_band² {d:.2e} of E², border σ {db:.2e}; windows: self-check '
          f'{check:.2e}, window σ + var_add vs bordered {dw:.2e}; {info["iters"]} iterations')
    assert d <= 2 * SIGMA_TOL and db <= SIGMA_TOL
    assert np.all(E_w <= E_grid * (1 + 1e-9)) and np.all(E_w > 0)
    assert np.max(va / E_ref[:P.n_g] ** 2) > 1e-3      # the term matters here


def test_op_rows_gain_the_border_term(gpu_available):
    P = _Pair(_build(65), S_NODES, NT)
    op = _op_rows(P.perm, P.n_g, np.random.default_rng(9))
    op_g = op.tocsc()[:, :P.n_g].tocsr()          # the grid columns are the first compact columns of both systems
    try:
        _, oe, _ = P.full.solver.cov_band_bordered(P.perm, P.k, op)
        _, oe_g, _ = P.grid.solver.cov_band(P.order_g, op_g)
        va, vb, op_add, _ = P.grid.solver.cov_border_solved(P.B, P.c_con, op_g, **SOLVE)
    finally:
        P.close()
    d = np.abs(op_add - (oe ** 2 - oe_g ** 2)).max() / (oe ** 2).max()
    print(f'op rows: op_add vs band op error² − grid-only op error² {d:.2e} of the largest op variance')
    assert d <= 2 * SIGMA_TOL
    assert np.array_equal(va, _case(65)['va']) and np.array_equal(vb, _case(65)['vb'])   # no effect on the columns


def test_refusals_leave_the_handle_usable(gpu_available, monkeypatch):
    P = _Pair(_build(65), S_NODES, NT)
    ref = _case(65)
    try:
        def still_answers(again=False):
            x, st = P.grid.solver.solve(np.ones(P.n_rows), precond=3, method=1, atol=1e-10, btol=1e-10)
            assert st['method'] == 1 and st['istop'] in (1, 2)
            if again:      # and the call itself returns the bits of an untouched handle
                va, vb, _, _ = P.grid.solver.cov_border_solved(P.B, P.c_con, **SOLVE)
                assert np.array_equal(va, ref['va']) and np.array_equal(vb, ref['vb'])

        with pytest.raises(NativeError, match=r'border column \d+') as e:       # too few iterations
            P.grid.solver.cov_border_solved(P.B, P.c_con, **dict(SOLVE, maxit=2))
        assert 'no output' in str(e.value)
        still_answers()
        bad = P.c_con.copy()                       # S indefinite
        bad[0, 0] = -1e12
        with pytest.raises(NativeError, match='not positive definite'):
            P.grid.solver.cov_border_solved(P.B, bad, **SOLVE)
        still_answers()
        ids = (np.arange(P.grid.n_data) % 3).astype(np.int32)      # an elimination on the handle
        P.grid.solver.set_data_bias(ids, np.ones(3))
        with pytest.raises(NativeError, match='elimination'):
            P.grid.solver.cov_border_solved(P.B, P.c_con, **SOLVE)
        P.grid.solver.set_data_bias(None, None)
        still_answers()
        with pytest.raises(NativeError, match='precond'):          # the dense preconditioner is not CGNR
            P.grid.solver.cov_border_solved(P.B, P.c_con, **dict(SOLVE, precond=2))
        # 65 columns pad to 128: (1792·128 + 3·128²)·8 = 2 228 224 bytes; 64 need 1 015 808
        monkeypatch.setenv('LSQ_BSOLVE_BUDGET', '1500000')
        with pytest.raises(NativeRefused, match='largest k that fits is 64'):
            P.grid.solver.cov_border_solved(P.B, P.c_con, **SOLVE)
        monkeypatch.delenv('LSQ_BSOLVE_BUDGET')
        still_answers()
        with pytest.raises(NativeError, match='data rows'):         # a row past the data rows
            Bb = sp.csc_matrix((np.ones(1), (np.array([P.n_rows - 1]), np.array([0]))), shape=(P.n_rows, 1))
            P.grid.solver.cov_border_solved(Bb, np.ones((1, 1)), **SOLVE)
        still_answers(again=True)
    finally:
        P.close()
    # the combined (triplet-formed) system has no CGNR operator
    with pytest.raises(NativeError, match='CGNR'):
        P2 = _build(5)
        try:
            P2[1].solver.cov_border_solved(sp.csc_matrix(np.ones((P2[1].n_data, 1))), np.ones((1, 1)), **SOLVE)
        finally:
            P2[1].close()


@functools.lru_cache(maxsize=None)
def _fits(name):
    g = golden(name)
    kw = _slope_kwargs(g) if 'slope' in name else golden_kwargs(g)
    fits = {}
    for bias in ('eliminate', 'columns'):
        for method, extra in (('band', {}), ('window', {'lsq_E_border_solve': True})):
            fits[bias, method] = LS.smooth_fit(data=golden_points(g), compute_E=True, lsq_E_border=True, lsq_bias=bias,
                                               lsq_E_method=method, **dict(kw, **extra))
    return fits


@pytest.mark.parametrize('name', ['sys_bias.npz', 'sys_slope.npz'])
def test_smooth_fit_window_with_biases_against_band(gpu_available, name):
    fits = _fits(name)
    for bias in ('eliminate', 'columns'):
        ref, out = fits[bias, 'band'], fits[bias, 'window']
        E, Er = out['E'], ref['E']
        assert set(E) == set(Er) and 'sigma_dzdt_lag1' in E
        t = out['timing']['E_border_solved']
        n_border = len(ref['m']['bias']['val']) + 2 * len(ref['m']['slope_bias'])
        assert t['k'] == n_border and t['iters'] > 0 and t['bytes'] > 0 and t['min_pivot'] > 0
        assert 'E_border_solved' not in ref['timing'] and 'E_window' in out['timing']
        for key in ('sigma_z0', 'sigma_dz', 'sigma_dzdt_lag1'):
            assert 'border' in E[key].approximate
            a, b = getattr(E[key], key), getattr(Er[key], key)
            ok = np.isfinite(b)
            assert np.array_equal(ok, np.isfinite(a)), (bias, key)
            d = _rel(a[ok], b[ok])
            print(f'{name} {bias} {key}: {d:.2e} (precond {t["precond"]}, {t["iters"]} iterations, asym {t["asym"]:.1e})')
            assert d <= SIGMA_TOL, (bias, key, d)
        assert set(E['sigma_bias']) == set(Er['sigma_bias'])
        for key in Er['sigma_bias']:
            x, y = np.asarray(E['sigma_bias'][key], float), np.asarray(Er['sigma_bias'][key], float)
            assert np.allclose(x, y, rtol=SIGMA_TOL, atol=0, equal_nan=True), (bias, key)
        assert set(E['sigma_slope_bias']) == set(Er['sigma_slope_bias']) and ('slope' in name) == bool(Er['sigma_slope_bias'])
        for sk, v in Er['sigma_slope_bias'].items():
            for comp in ('slope_x', 'slope_y'):
                assert abs(E['sigma_slope_bias'][sk][comp] - v[comp]) <= SIGMA_TOL * abs(v[comp]), (bias, sk, comp)


def test_smooth_fit_window_sigma_matches_the_reference(gpu_available):
    """sys_bias against the reference's compute_E with an exact R⁻¹, at the bound tests/test_gpu_border.py
    holds the band path to (1e-8), and against its own truncated result (10 × the recorded difference)."""
    g = golden('sys_bias_E.npz')
    E = _fits('sys_bias.npz')['eliminate', 'window']['E']
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
