#!/usr/bin/env python3
"""Cost of the slope elimination (csrc/slope.inc) at C4 size against the bias-only step, in one process.

On the synthetic C4 system (synthetic.points('c4'), 2 M points, all rows kept) half the points,
picked at random, belong to 40 "DEM strips" (slope sensors: bins of x), each with 12 bias IDs (bins
of time); the other half share 12 further bias IDs (bins of time) and lie outside every slope group.
c = 1 / 0.5 for every bias, 1 / 10 for every slope; u is the strip's centred (x, y) in km.

1. lsq_iterate, CGNR + block-Jacobi, with the biases only and with biases and slopes: rounds that
   alternate the two on the same handle, each round a warm-up batch and then `--steps` timed
   iterations (device events inside the library, stats['time_s']).  The ratio of the two medians is
   the cost of the slopes; the plain step (no biases) is measured in the same rounds.
2. each kernel of the step with slopes, timed by device events inside real iterations
   (lsq_profile_data_slope), against its share of the byte model at 0.43 × 8 TB/s, the fraction of
   peak the existing data-row kernels reach.
3. a converged solve (atol = btol = 1e-12) with the block-Jacobi and with the multigrid
   preconditioner, with biases only and with slopes: the iteration counts.

Usage: python tools/slope_step.py OUT.json [--config c4] [--steps 200] [--rounds 5] [--no-solves]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_SENSORS, IDS_PER_SENSOR = 40, 12
TOL = dict(atol=1e-12, btol=1e-12, conlim=1e12)


def bins(v, n):
    v = np.asarray(v, float)
    return np.minimum((n * (v - v.min()) / (v.max() - v.min())).astype(np.int64), n - 1)


def layout(D, rng):
    """(ids, c, grp, u, cs) of the measurement."""
    dem = rng.random(D.size) < 0.5
    grp = np.where(dem, bins(D.x, N_SENSORS), -1).astype(np.int32)
    tb = bins(D.time, IDS_PER_SENSOR)
    ids = np.where(dem, grp * IDS_PER_SENSOR + tb, N_SENSORS * IDS_PER_SENSOR + tb).astype(np.int32)
    u = np.zeros((D.size, 2))
    for g in range(N_SENSORS):
        mine = grp == g
        u[mine, 0] = (D.x[mine] - D.x[mine].mean()) / 1000
        u[mine, 1] = (D.y[mine] - D.y[mine].mean()) / 1000
    return ids, np.full((N_SENSORS + 1) * IDS_PER_SENSOR, 2.0), grp, u, np.full((N_SENSORS, 2), 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('--config', default='c4')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-solves', action='store_true')
    a = ap.parse_args()

    import lssurf_amd as LS
    from lssurf_amd import synthetic
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    from lssurf_amd.smooth_fit import FitSystem

    D, kw = synthetic.points(a.config)
    S = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw)
    keep = reference_epoch_keep_cols(S['G_data'].col_N, S['grids']['dz'], kw['reference_epoch'])
    w = np.abs(1. / np.concatenate((S['Ed'], S['Ec'])))
    rhs = np.zeros(w.size)
    rhs[:S['data'].size] = S['data'].z
    fs = FitSystem(S['G_data'], S['Gc'], keep, S['Gc'].col_N, grids=S['grids'])
    sol = fs.solver
    sol.set_row_weight(w)
    sol.set_row_mask(np.ones(w.size, bool))
    ids, c, grp, u, cs = layout(S['data'], np.random.default_rng(5))
    rate = 0.43 * 8e12
    res = {'config': a.config, 'n_points': int(fs.n_data), 'n_cols': int(keep.size), 'steps': a.steps,
           'rounds': a.rounds, 'slope_sensors': N_SENSORS, 'bias_ids': int(c.size),
           'points_in_groups': int((grp >= 0).sum()),
           'timing': 'device events around the iterations (stats time_s), medians of alternating rounds in one '
                     'process; kernels: device events between the launches inside real iterations',
           'budget_rate_bytes_per_s': rate}

    def step(mode):
        sol.set_data_bias(ids, c) if mode else sol.set_data_bias(None, None)   # drops the captured batch
        if mode == 2:
            sol.set_data_slope(grp, u, cs)
        sol.iterate(rhs, 32, precond=3, method=1, b_rows=fs.n_data)       # init + warm-up
        st = sol.iterate(rhs, a.steps, precond=3, method=1, b_rows=fs.n_data)
        return 1e3 * st['time_s'] / a.steps, st['bytes_per_iter']

    try:
        t, by = {0: [], 1: [], 2: []}, {}
        for _ in range(a.rounds):
            for mode in (0, 1, 2):
                ms, by[mode] = step(mode)
                t[mode].append(ms)
        med = {m: float(np.median(t[m])) for m in t}
        res['step'] = {'step_ms_plain': med[0], 'step_ms_bias': med[1], 'step_ms_slope': med[2],
                       'step_ms_plain_all': t[0], 'step_ms_bias_all': t[1], 'step_ms_slope_all': t[2],
                       'ratio_slope_over_bias': med[2] / med[1],
                       'elimination_us_bias': 1e3 * (med[1] - med[0]), 'elimination_us_slope': 1e3 * (med[2] - med[0]),
                       'model_bytes_bias': float(by[1] - by[0]), 'model_bytes_slope': float(by[2] - by[0]),
                       'budget_us_bias': 1e6 * float(by[1] - by[0]) / rate,
                       'budget_us_slope': 1e6 * float(by[2] - by[0]) / rate}
        print(res['step'], flush=True)
        # the live state of the last round carries the slopes
        prof = sol.profile_data_slope(reps=50, precond=3)
        res['kernels'] = {k: {'us': 1e3 * ms, 'model_bytes': b, 'budget_us': 1e6 * b / rate,
                              'over_budget': 1e3 * ms / max(1e6 * b / rate, 1e-9)} for k, (ms, b) in prof.items()}
        print(res['kernels'], flush=True)
        if not a.no_solves:
            for precond, label in ((3, 'block_jacobi'), (4, 'multigrid')):
                iters = {}
                for mode, name in ((1, 'bias'), (2, 'slope')):
                    sol.set_data_bias(ids, c)
                    if mode == 2:
                        sol.set_data_slope(grp, u, cs)
                    if not sol.cg_available(precond)[0]:
                        continue
                    _, st = sol.solve(rhs, precond=precond, method=1, maxit=200000, b_rows=fs.n_data, **TOL)
                    iters[name] = {'iters': int(st['iters']), 'istop': int(st['istop']), 'time_s': float(st['time_s'])}
                    print(label, name, iters[name], flush=True)
                res['solve_' + label] = iters
    finally:
        fs.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
