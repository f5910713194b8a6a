#!/usr/bin/env python3
"""Cost of the joint elimination of sensor grids beside biases and slopes (csrc/sgrid.inc,
lsq_set_sensor_grids_joint) at C4 size, in one process, on the frame of tools/sgrid_step.py.

On the synthetic C4 system (synthetic.points('c4'), 2 M points, all rows kept) half the points,
picked at random, belong to 40 "DEM strips" (sensors 1 … 40: bins of x).  Each strip has a bias grid of
setup_sensor_grid_bias with `--spacing` (1000 m: 420 … 525 nodes; magnitude rows expected_rms 1,
curvature rows expected_rms_grad2 1e-5), one bias ID (c = 1 / 0.5) and one slope group (c = 1 / 10, u
the strip's centred (x, y) in km): three dense nodes per block.  The other half carries `rgt × cycle`
biases (12 × 12 IDs: bins of y and of time) outside every grid and group.

1. lsq_iterate, CGNR + block-Jacobi: rounds that alternate, on the same handle, the plain step, the
   step with biases and slopes only, with the grids only (no biases) and the joint step; each round a
   warm-up batch and then `--steps` timed iterations (device events inside the library,
   stats['time_s']).  The joint elimination's cost is set against the sum of the two single ones.
2. each kernel of the joint step, timed by device events inside real iterations: the four block
   kernels (lsq_profile_sensor_grids) and the bias path's (lsq_profile_data_slope), the stages of the
   two profiles that span the other path's launches taken off each other (untangle), against their
   shares of the byte model at 0.43 × 8 TB/s, the fraction of peak the existing data-row kernels reach.
   Then the joint step once more with one wave per dense-node list (LSQ_SG_SEG=0): what the segments
   of the long lists are measured against.
3. a converged solve (atol = btol = 1e-12) with block-Jacobi and with the multigrid preconditioner,
   with biases and slopes only and jointly: iterations, solve time and the per-solve set-up
   (stats['setup_s']: with grids it holds the assembly and factorisation of every M_s).

The record is rewritten after every stage, so a run that is cut short keeps what it measured.

Usage: python tools/sgrid_joint_step.py OUT.json [--config c4] [--steps 200] [--rounds 3] [--spacing 1000]
                                                 [--maxit 20000] [--no-solves]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sgrid_step import N_SENSORS, TOL, bins, layout   # noqa: E402

N_RGT = N_CYCLE = 12
MODES = ('plain', 'bias_slope', 'grids', 'joint')


def bias_layout(D):
    """(ids, c, grp, u, cs) beside the grids of sgrid_step.layout (which assigns D.sensor)."""
    dem = D.sensor > 0
    grp = np.where(dem, D.sensor - 1, -1).astype(np.int32)
    loose = N_SENSORS + bins(D.y, N_RGT) * N_CYCLE + bins(D.time, N_CYCLE)
    ids = np.where(dem, grp, loose).astype(np.int32)
    u = np.zeros((D.size, 2))
    for g in range(N_SENSORS):
        mine = grp == g
        u[mine, 0] = (D.x[mine] - D.x[mine].mean()) / 1000
        u[mine, 1] = (D.y[mine] - D.y[mine].mean()) / 1000
    return ids, np.full(N_SENSORS + N_RGT * N_CYCLE, 2.0), grp, u, np.full((N_SENSORS, 2), 0.1)


def untangle(blocks, path):
    """The two profiles of the joint step with their overlapping stages taken off each other.  The step
    launches the bias path's reduce, the blocks' reduce, the bias path's apply, the blocks' apply.
    lsq_profile_sensor_grids marks the blocks' launches: its first stage spans the bias path's reduce,
    its fourth the bias path's apply.  lsq_profile_data_slope marks the bias path's: its apply stage
    spans the blocks' reduce."""
    blocks, path = dict(blocks), dict(path)
    blocks['btd'] = (blocks['btd'][0] - sum(path[k][0] for k in ('chunk', 'rank', 'group')), blocks['btd'][1])
    path['apply'] = (path['apply'][0] - sum(blocks[k][0] for k in ('btd', 'trsv_t', 'trsv')), path['apply'][1])
    blocks['apply'] = (blocks['apply'][0] - path['apply'][0], blocks['apply'][1])
    return blocks, path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('--config', default='c4')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
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
    ids, c, grp, u, cs = bias_layout(S['data'])
    print(f'host objects in {time.time() - tic:.0f} s; grids of {sg["n_nodes"].min()} … {sg["n_nodes"].max()} nodes',
          flush=True)
    fs = FitSystem(S['G_data'], S['Gc'], keep, S['Gc'].col_N, grids=S['grids'])
    sol = fs.solver
    sol.set_row_weight(w)
    sol.set_row_mask(np.ones(w.size, bool))
    rate = 0.43 * 8e12
    rows = np.bincount(sg['grid'][sg['grid'] >= 0], minlength=N_SENSORS)
    res = {'config': a.config, 'n_points': int(fs.n_data), 'n_cols': int(keep.size), 'steps': a.steps,
           'rounds': a.rounds, 'sensors': N_SENSORS, 'spacing': a.spacing,
           'nodes_per_grid': [int(n) for n in sg['n_nodes']], 'grid_unknowns': int(sg['n_nodes'].sum()),
           'dense_nodes_per_grid': 3, 'points_in_grids': int((sg['grid'] >= 0).sum()),
           'rows_per_grid': [int(rows.min()), int(rows.max())], 'bias_ids': int(c.size),
           'loose_bias_ids': N_RGT * N_CYCLE,
           'timing': 'device events around the iterations (stats time_s), medians of alternating rounds in one '
                     'process; kernels: device events between the launches inside real iterations',
           'budget_rate_bytes_per_s': rate}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)

    def set_mode(mode):   # every call drops the captured batch
        sol.set_sensor_grids(None, None, None, None, None)
        sol.set_data_bias(None, None)
        if mode in ('bias_slope', 'joint'):
            sol.set_data_bias(ids, c)
            sol.set_data_slope(grp, u, cs)
        if mode in ('grids', 'joint'):
            sol.set_sensor_grids(sg['grid'], sg['node'], sg['wt'], sg['n_nodes'], sg['K'], joint=mode == 'joint')

    def step(mode):
        set_mode(mode)
        sol.iterate(rhs, 32, precond=3, method=1, b_rows=fs.n_data)       # init + warm-up
        st = sol.iterate(rhs, a.steps, precond=3, method=1, b_rows=fs.n_data)
        return 1e3 * st['time_s'] / a.steps, st['bytes_per_iter']

    try:
        t, by = {m: [] for m in MODES}, {}
        for _ in range(a.rounds):
            for mode in MODES:                                            # 'joint' last: its live state is profiled
                ms, by[mode] = step(mode)
                t[mode].append(ms)
        med = {m: float(np.median(t[m])) for m in t}
        res['step'] = {'step_ms': med, 'step_ms_all': t,
                       'elimination_us': {m: 1e3 * (med[m] - med['plain']) for m in MODES[1:]},
                       'joint_over_sum_of_parts': (med['joint'] - med['plain']) /
                       max(med['bias_slope'] + med['grids'] - 2 * med['plain'], 1e-12),
                       'model_bytes': {m: float(by[m] - by['plain']) for m in MODES[1:]},
                       'budget_us': {m: 1e6 * float(by[m] - by['plain']) / rate for m in MODES[1:]}}
        print(res['step'], flush=True)
        save()
        blocks = sol.profile_sensor_grids(reps=50, precond=3)
        path = sol.profile_data_slope(reps=50, precond=3)
        blocks, path = untangle(blocks, path)
        kern = {'sgrid_' + k: v for k, v in blocks.items()}
        kern.update({'bias_' + k: v for k, v in path.items()})
        res['kernels'] = {k: {'us': 1e3 * ms, 'model_bytes': b, 'budget_us': 1e6 * b / rate,
                              'over_budget': 1e3 * ms / max(1e6 * b / rate, 1e-9)} for k, (ms, b) in kern.items()}
        print(res['kernels'], flush=True)
        save()
        # the same joint step with one wave per dense-node list (LSQ_SG_SEG=0, read when the grids are set):
        # what cutting the long lists into segments is measured against
        os.environ['LSQ_SG_SEG'] = '0'
        try:
            ms, _ = step('joint')
            b0, p0 = untangle(sol.profile_sensor_grids(reps=50, precond=3), sol.profile_data_slope(reps=50, precond=3))
        finally:
            del os.environ['LSQ_SG_SEG']
        res['one_wave_per_list'] = {'step_ms_joint': ms, 'elimination_us': 1e3 * (ms - med['plain']),
                                    'sgrid_btd_us': 1e3 * b0['btd'][0], 'sgrid_btd_budget_us': 1e6 * b0['btd'][1] / rate}
        print(res['one_wave_per_list'], flush=True)
        save()
        if not a.no_solves:
            for precond, label in ((3, 'block_jacobi'), (4, 'multigrid')):
                iters = {}
                for mode in ('bias_slope', 'joint'):
                    set_mode(mode)
                    if not sol.cg_available(precond)[0]:
                        continue
                    _, st = sol.solve(rhs, precond=precond, method=1, maxit=a.maxit, b_rows=fs.n_data, **TOL)
                    iters[mode] = {'iters': int(st['iters']), 'istop': int(st['istop']), 'time_s': float(st['time_s']),
                                   'setup_s': float(st.get('setup_s', 0.))}
                    print(label, mode, iters[mode], flush=True)
                    res['solve_' + label] = iters
                    save()
    finally:
        fs.close()
    save()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
