#!/usr/bin/env python3
"""Cost and accuracy of lsq_cov_border_solved (csrc/bsolve.inc), the border term of compute_E where no
band factor fits, in one process.  Three stages, each optional; the record is rewritten after every
stage, so a run that is cut short keeps what it measured.

tests   the cases of tests/test_gpu_border_solved.py (17 × 17 × 6, borders of 1, 5, 65 and the mixed
        134): the relative σ deviation of sqrt(E_window² + var_add) and sqrt(var_border) from
        cov_band_bordered and from the host inverse, for the first call and for the re-weighted one.
        Ten times the largest deviation from cov_band_bordered is the tests' SIGMA_TOL.
c1      the frame of tools/border_e.py (synthetic.points('c1'), k = 64 and 512 bias IDs dealt out at
        random): cov_band_bordered on the combined system beside cov_band (the exact (N⁻¹)_jj, standing in
        for the windows) plus cov_border_solved on the grid-only system: seconds of each, the σ agreement.
big     synthetic.points('c4') (or --big c3) with the 144 `rgt × cycle` biases of tools/sgrid_joint_step.py
        (12 bins of y × 12 of time, expected size 0.5), all rows kept: iterations and seconds of the
        solves (per solve and in all), the steps behind them apart, the var_add kernel (device events)
        against its byte model — one read of Z and n·k_pad² flops —, asym, the smallest pivot and Z's bytes.
        There is no band factor to compare σ with at this size; asym / pivot is the run-time measure.
e2e     smooth_fit end to end at --e2e size (c3) with the same 144 biases (lsq_bias='eliminate', two outer
        iterations) and compute_E through lsq_E_border_solve: seconds of the fit, the windows and the border.

Solves: CGNR with the multigrid preconditioner where the system has it, else block-Jacobi, atol = btol =
1e-12 (smooth_fit's defaults).  Times are host wall clock around work that ends in a stream
synchronise (the library's info), except where device events are named.

Usage: python tools/border_solved.py OUT.json [--stages tests c1 big e2e] [--c1-k 64 512] [--big c4] [--e2e c3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-12


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def stage_tests():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_border_solved import CASES, _case
    res, worst = {}, 0.0
    for k in CASES:
        r = _case(k)
        n_g = r['n_g']
        E = np.concatenate((np.sqrt(r['E_win'] ** 2 + r['va']), np.sqrt(r['vb'])))
        E_rw = np.concatenate((np.sqrt((r['E_win'] / 1.5) ** 2 + r['va_rw']), np.sqrt(r['vb_rw'])))
        c = {'k': r['k'], 'iters': r['info']['iters'], 'iters_max': r['info']['iters_max'],
             'solve_s': r['info']['solve_us'] * 1e-6, 'asym': r['info']['asym'], 'min_pivot': r['info']['min_pivot']}
        for name, sel in (('grid', slice(0, n_g)), ('border', slice(n_g, None))):
            c[name] = {'vs_band_bordered': _rel(E[sel], r['E_ref'][sel]), 'vs_host_inverse': _rel(E[sel], r['E_host'][sel]),
                       'reweighted_vs_band_bordered': _rel(E_rw[sel] * 1.5, r['E_ref'][sel])}
            worst = max(worst, c[name]['vs_band_bordered'], c[name]['reweighted_vs_band_bordered'])
        res[str(k)] = c
        print('tests', k, c, flush=True)
    res['largest_vs_band_bordered'] = worst
    res['SIGMA_TOL'] = 10 * worst
    return res


def _fit_objects(LS, D, kw, ids=None):
    """(combined fit objects or None, grid-only fit objects) of the points; ids: the bias ID per point"""
    Sg = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw)
    if ids is None:
        return None, Sg
    Db = D.copy()
    Db.assign(cycle=np.asarray(ids, float), sigma_corr=np.full(D.size, 0.5))
    Sb = LS.smooth_fit(data=Db, return_fit_objects=True, VERBOSE=False, bias_params=['cycle'], lsq_bias='columns', **kw)
    return Sb, Sg


def _border_solved(fs, w, B, c_con, opts):
    """cov_border_solved on the grid-only FitSystem (weights set here): the info, seconds, outputs"""
    fs.solver.set_row_weight(np.ascontiguousarray(w[:fs.n_data + fs.n_con]))
    fs.solver.set_row_mask(np.ones(fs.n_data + fs.n_con, bool))
    mg = fs.multigrid_available()
    opts = dict(opts, precond=4 if mg else 3)
    tic = time.time()
    va, vb, _, info = fs.solver.cov_border_solved(B, c_con, **opts)
    return va, vb, info, time.time() - tic, opts['precond']


def stage_c1(ks):
    import lssurf_amd as LS
    from lssurf_amd import synthetic
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    from lssurf_amd.errors import band_order, bordered_band_order, split_border
    from lssurf_amd.smooth_fit import FitSystem
    D, kw = synthetic.points('c1')
    rng = np.random.default_rng(20261020)
    res = {'config': 'c1', 'n_points': int(D.size)}
    for k in ks:
        Sb, Sg = _fit_objects(LS, D, kw, rng.permutation(D.size) % k)
        n_grid = int(Sb['grids']['dz'].col_N)
        keep = reference_epoch_keep_cols(Sb['G_data'].col_N, Sb['grids']['dz'], kw['reference_epoch'])
        keep_g = keep[keep < n_grid]
        w = np.abs(1. / np.concatenate((Sb['Ed'], Sb['Ec'])))
        perm, nb = bordered_band_order(Sb['grids'], keep, n_grid)
        full = FitSystem(Sb['G_data'], Sb['Gc'], keep, Sb['Gc'].col_N)
        try:
            full.solver.set_row_weight(w)
            full.solver.cov_band_bordered(perm, nb)   # warm-up: code objects, the full CSR
            tic = time.time()
            E_ref, _, binfo = full.solver.cov_band_bordered(perm, nb)
            t_band = time.time() - tic
        finally:
            full.close()
        G_grid, Gc_grid, B, c_con = split_border(Sb['G_data'], Sb['Gc'], Sb['Ec'], keep, n_grid,
                                                 grid_ops=(Sg['G_data'], Sg['Gc']))
        fs = FitSystem(G_grid, Gc_grid, keep_g, n_grid, grids=Sg['grids'])
        try:
            va, vb, info, t_solved, pc = _border_solved(fs, w, B, c_con, dict(atol=TOL, btol=TOL, conlim=1e12,
                                                                            maxit=50 * keep_g.size))
            tic = time.time()
            E_grid, _, _ = fs.solver.cov_band(band_order(Sg['grids'], keep_g))
            t_grid = time.time() - tic
        finally:
            fs.close()
        E = np.concatenate((np.sqrt(E_grid ** 2 + va), np.sqrt(vb)))
        n_g = keep_g.size
        c = {'n_cols': int(keep.size), 'n_border': int(nb), 'band_bordered_s': t_band,
             'band_bordered_border_phase_s': 1e-6 * int(binfo[8]), 'grid_only_cov_band_s': t_grid,
             'border_solved_s': t_solved, 'precond': pc, 'info': info,
             'sigma_grid_vs_band_bordered': _rel(E[:n_g], E_ref[:n_g]),
             'sigma_border_vs_band_bordered': _rel(E[n_g:], E_ref[n_g:]),
             'seconds_per_solve': info['solve_us'] * 1e-6 / nb, 'iters_per_solve': info['iters'] / nb}
        res[f'k{k}'] = c
        print('c1', k, c, flush=True)
    return res


def stage_big(config):
    import lssurf_amd as LS
    from lssurf_amd import synthetic
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    from lssurf_amd.smooth_fit import FitSystem
    from sgrid_step import bins
    import scipy.sparse as sp
    tic = time.time()
    D, kw = synthetic.points(config)
    _, Sg = _fit_objects(LS, D, kw)
    data = Sg['data']
    n_rgt = n_cycle = 12
    ids = bins(data.y, n_rgt) * n_cycle + bins(data.time, n_cycle)
    k = n_rgt * n_cycle
    # the border as errors.split_border makes it for `cycle`-type biases: a 1 per data row in its ID's
    # column, and the bias constraint rows' share 1 / expected² on the diagonal
    B = sp.csc_matrix((np.ones(data.size), (np.arange(data.size), ids)), shape=(data.size, k))
    c_con = np.eye(k) / 0.5 ** 2
    n_grid = int(Sg['grids']['dz'].col_N)
    keep_g = reference_epoch_keep_cols(Sg['G_data'].col_N, Sg['grids']['dz'], kw['reference_epoch'])
    w = np.abs(1. / np.concatenate((Sg['Ed'], Sg['Ec'])))
    host_s = time.time() - tic
    fs = FitSystem(Sg['G_data'], Sg['Gc'], keep_g, n_grid, grids=Sg['grids'])
    try:
        va, vb, info, t_solved, pc = _border_solved(fs, w, B, c_con, dict(atol=TOL, btol=TOL, conlim=1e12,
                                                                        maxit=20000))
        rhs = np.zeros(w.size)      # the plain fit's solve on the same handle, for the iteration count
        rhs[:data.size] = data.z
        _, st = fs.solver.solve(rhs, atol=TOL, btol=TOL, conlim=1e12, maxit=20000, precond=pc, method=1,
                                b_rows=fs.n_data)
    finally:
        fs.close()
    n, kpad = int(keep_g.size), info['k_pad']
    npad = -(-n // 64) * 64
    z_bytes, flops = npad * kpad * 8, float(npad) * kpad * kpad   # the triangle halves 2·n·k²
    ker_s = info['var_add_kernel_us'] * 1e-6
    return {'config': config, 'n_points': int(data.size), 'n_cols': n, 'k': k, 'host_objects_s': host_s, 'precond': pc,
            'call_s': t_solved, 'info': info, 'seconds_per_solve': info['solve_us'] * 1e-6 / k,
            'iters_per_solve': info['iters'] / k, 'plain_fit_solve': {'iters': int(st['iters']), 'time_s': st['time_s'],
                                                                     'setup_s': st['setup_s']},
            'steps_s': {'T': info['T_us'] * 1e-6, 'S_and_factor': info['S_us'] * 1e-6, 'var_add': info['var_add_us'] * 1e-6,
                        'op_add': info['op_add_us'] * 1e-6},
            'var_add_kernel': {'seconds': ker_s, 'z_bytes': z_bytes, 'flops_model': flops,
                               'bytes_per_s': z_bytes / ker_s if ker_s else None,
                               'flops_per_s': flops / ker_s if ker_s else None},
            'asym': info['asym'], 'min_pivot': info['min_pivot'], 'asym_over_pivot': info['asym'] / info['min_pivot'],
            'sigma_bias_range': [float(np.sqrt(vb.min())), float(np.sqrt(vb.max()))],
            'var_add_max': float(va.max())}


def stage_e2e(config):
    import lssurf_amd as LS
    from lssurf_amd import synthetic
    from sgrid_step import bins
    D, kw = synthetic.points(config)
    D.assign(cycle=(bins(D.y, 12) * 12 + bins(D.time, 12)).astype(float), sigma_corr=np.full(D.size, 0.5))
    tic = time.time()
    out = LS.smooth_fit(data=D, bias_params=['cycle'], lsq_bias='eliminate', compute_E=True, lsq_E_border=True,
                        lsq_E_border_solve=True, VERBOSE=False, **dict(kw, max_iterations=2))
    t = out['timing']
    sb = np.asarray(out['E']['sigma_bias']['val'], float)
    return {'config': config, 'n_points': int(D.size), 'total_s': time.time() - tic, 'fit_iteration_s': t['iteration'],
            'lsq_iters_per_solve': t['lsq_iters_per_solve'], 'propagate_errors_s': t['propagate_errors'],
            'E_window': t['E_window'], 'E_border_solved': t['E_border_solved'],
            'sigma_bias_range': [float(sb.min()), float(sb.max())], 'approximate': out['E']['sigma_z0'].approximate}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('--stages', nargs='+', default=['tests', 'c1', 'big', 'e2e'],
                    choices=['tests', 'c1', 'big', 'e2e'])
    ap.add_argument('--c1-k', type=int, nargs='+', default=[64, 512])
    ap.add_argument('--big', default='c4')
    ap.add_argument('--e2e', default='c3')
    a = ap.parse_args()
    res = {'timing': 'host wall clock around synchronised work (the library\'s info); var_add_kernel: device events',
           'solve_tolerance': TOL}
    if os.path.exists(a.out):      # stages of an earlier run stay
        with open(a.out) as f:
            res.update(json.load(f))

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)

    for stage in a.stages:
        key = {'big': a.big, 'e2e': a.e2e + '_end_to_end'}.get(stage, stage)
        res[key] = {'tests': stage_tests, 'c1': lambda: stage_c1(a.c1_k), 'big': lambda: stage_big(a.big),
                    'e2e': lambda: stage_e2e(a.e2e)}[stage]()
        save()


if __name__ == '__main__':
    main()
