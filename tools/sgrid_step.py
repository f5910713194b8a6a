#!/usr/bin/env python3
"""Cost of the sensor grids' elimination (csrc/sgrid.inc) at C4 size against the plain step, in one process.

On the synthetic C4 system (synthetic.points('c4'), 2 M points, all rows kept) half the points,
picked at random, belong to 40 "DEM strips" (sensors 1 … 40: bins of x); each strip gets a bias grid
of setup_sensor_grid_bias with `--spacing` (1000 m: about 500 nodes), held by magnitude rows
(expected_rms 1) and curvature rows (expected_rms_grad2 1e-5).

1. lsq_iterate, CGNR + block-Jacobi, plain and with the grids: rounds that alternate the two on the
   same handle, each round a warm-up batch and then `--steps` timed iterations (device events inside
   the library, stats['time_s']).  The difference of the two medians is the cost of the elimination.
2. each kernel of the step, timed by device events inside real iterations
   (lsq_profile_sensor_grids), against its share of the byte model at 0.43 × 8 TB/s, the fraction of
   peak the existing data-row kernels reach.
3. a converged solve (atol = btol = 1e-12) with the block-Jacobi and with the multigrid
   preconditioner, plain and with the grids: the iteration counts, the solve time and the per-solve
   set-up (stats['setup_s']: with grids it holds the assembly and factorisation of every M_s).

The record is rewritten after every stage, so a run that is cut short keeps what it measured.

Usage: python tools/sgrid_step.py OUT.json [--config c4] [--steps 200] [--rounds 5] [--spacing 1000]
                                           [--maxit 20000] [--no-solves]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_SENSORS = 40
TOL = dict(atol=1e-12, btol=1e-12, conlim=1e12)


def bins(v, n):
    v = np.asarray(v, float)
    return np.minimum((n * (v - v.min()) / (v.max() - v.min())).astype(np.int64), n - 1)


def layout(D, spacing, rng):
    """The device form (sensor_grid_device_form) of the measurement's grids."""
    from lssurf_amd.lin_op import lin_op
    from lssurf_amd.setup_sensor_grid_bias import sensor_grid_device_form, setup_sensor_grid_bias
    dem = rng.random(D.size) < 0.5
    D.assign(sensor=np.where(dem, 1 + bins(D.x, N_SENSORS), 0).astype(float))
    grids, ops, sensor_of = {}, [], {}
    G = lin_op(col_0=0, col_N=0, name='data')
    for s in range(1, N_SENSORS + 1):
        name = setup_sensor_grid_bias(D, grids, G, ops, sensor=float(s), spacing=spacing, expected_rms=1.0,
                                      expected_rms_grad2=1e-5)
        sensor_of[name] = float(s)
    for op in ops:
        if op.prior is None:
            op.prior = np.zeros(np.shape(op.expected))
    return sensor_grid_device_form(D, grids, sensor_of, ops)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('--config', default='c4')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--spacing', type=float, default=1000.)
    ap.add_argument('--maxit', type=int, default=20000)
    ap.add_argument('--no-solves', action='store_true')
    a = ap.parse_args()

    import lssurf_amd as LS
    from lssurf_amd import synthetic
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    from lssurf_amd.smooth_fit import FitSystem

    tic = time.time()
    D, kw = synthetic.points(a.config)
    S = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw)
    keep = reference_epoch_keep_cols(S['G_data'].col_N, S['grids']['dz'], kw['reference_epoch'])
    w = np.abs(1. / np.concatenate((S['Ed'], S['Ec'])))
    rhs = np.zeros(w.size)
    rhs[:S['data'].size] = S['data'].z
    sg = layout(S['data'], a.spacing, np.random.default_rng(5))
    print(f'host objects in {time.time() - tic:.0f} s; grids of {sg["n_nodes"].min()} … {sg["n_nodes"].max()} nodes',
          flush=True)
    fs = FitSystem(S['G_data'], S['Gc'], keep, S['Gc'].col_N, grids=S['grids'])
    sol = fs.solver
    sol.set_row_weight(w)
    sol.set_row_mask(np.ones(w.size, bool))
    rate = 0.43 * 8e12
    res = {'config': a.config, 'n_points': int(fs.n_data), 'n_cols': int(keep.size), 'steps': a.steps,
           'rounds': a.rounds, 'sensors': N_SENSORS, 'spacing': a.spacing,
           'nodes_per_grid': [int(n) for n in sg['n_nodes']], 'grid_unknowns': int(sg['n_nodes'].sum()),
           'points_in_grids': int((sg['grid'] >= 0).sum()),
           'timing': 'device events around the iterations (stats time_s), medians of alternating rounds in one '
                     'process; kernels: device events between the launches inside real iterations',
           'budget_rate_bytes_per_s': rate}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)

    def set_grids(on):
        if on:
            sol.set_sensor_grids(sg['grid'], sg['node'], sg['wt'], sg['n_nodes'], sg['K'])
        else:
            sol.set_sensor_grids(None, None, None, None, None)

    def step(mode):
        set_grids(mode)                                                   # drops the captured batch
        sol.iterate(rhs, 32, precond=3, method=1, b_rows=fs.n_data)       # init + warm-up
        st = sol.iterate(rhs, a.steps, precond=3, method=1, b_rows=fs.n_data)
        return 1e3 * st['time_s'] / a.steps, st['bytes_per_iter']

    try:
        t, by = {0: [], 1: []}, {}
        for _ in range(a.rounds):
            for mode in (0, 1):
                ms, by[mode] = step(mode)
                t[mode].append(ms)
        med = {m: float(np.median(t[m])) for m in t}
        res['step'] = {'step_ms_plain': med[0], 'step_ms_grids': med[1],
                       'step_ms_plain_all': t[0], 'step_ms_grids_all': t[1],
                       'ratio_grids_over_plain': med[1] / med[0],
                       'elimination_us': 1e3 * (med[1] - med[0]),
                       'model_bytes': float(by[1] - by[0]), 'budget_us': 1e6 * float(by[1] - by[0]) / rate}
        print(res['step'], flush=True)
        save()
        # the live state of the last round carries the grids
        prof = sol.profile_sensor_grids(reps=50, precond=3)
        res['kernels'] = {k: {'us': 1e3 * ms, 'model_bytes': b, 'budget_us': 1e6 * b / rate,
                              'over_budget': 1e3 * ms / max(1e6 * b / rate, 1e-9)} for k, (ms, b) in prof.items()}
        print(res['kernels'], flush=True)
        save()
        if not a.no_solves:
            for precond, label in ((3, 'block_jacobi'), (4, 'multigrid')):
                iters = {}
                for mode, name in ((0, 'plain'), (1, 'grids')):
                    set_grids(mode)
                    if not sol.cg_available(precond)[0]:
                        continue
                    _, st = sol.solve(rhs, precond=precond, method=1, maxit=a.maxit, b_rows=fs.n_data, **TOL)
                    iters[name] = {'iters': int(st['iters']), 'istop': int(st['istop']), 'time_s': float(st['time_s']),
                                   'setup_s': float(st.get('setup_s', 0.))}
                    print(label, name, iters[name], flush=True)
                    res['solve_' + label] = iters
                    save()
    finally:
        fs.close()
    save()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
