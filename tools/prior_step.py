#!/usr/bin/env python3
"""Cost of the extra rows' step (csrc/xrows.inc) at C4 size, in one process.

On the synthetic C4 system (synthetic.points('c4'), all rows kept) a synthetic tile-edge frame is
laid on the dz grid: the 3 km strips along the edges of a central 80 km tile at the grid's own
resolution, every non-reference epoch, one prior row per node and epoch (1 at the node, −1 at its
reference-epoch column), σ = 0.1, priors N(0, 0.05).  Two handles live side by side, one without
and one with these extra rows:

1. lsq_iterate, CGNR + block-Jacobi: rounds that alternate the two handles, each round a warm-up
   batch and then `--steps` timed iterations (device events inside the library, stats['time_s']).
   The extra time per step is the difference of the two medians of the same run, set against the
   step's byte model (xr_step_bytes, lsq_extra_rows_info) over 0.43 × 8 TB/s, the fraction of peak
   the existing data-row kernels reach.  Then the two kernels' own times: device events between
   the launches of real iterations on the live state (lsq_profile_extra_rows), k_xr_fwd and
   k_xr_atq apart, each set against its share of xr_step_bytes, with the data rows' Ad·p before
   them and the node gather behind them for scale.
2. a converged block-Jacobi solve (atol = btol = 1e-12) on each: the iteration counts.
3. the device bytes of the extra rows and their transpose.
4. (--mg OUT_MG.json) the multigrid leg: the prior handle is formed with the rows' lumping requested
   (FitSystem(extra_mg=True); the block-Jacobi numbers above do not depend on it).  Converged solves
   (atol = btol = 1e-12) of block-Jacobi with priors, multigrid with lumped priors and multigrid
   without priors: iterations, time_s, setup_s.  The device time of one lumping pass of the set-up
   (k_mg_lump_xr with its long-node kernel, lsq_profile_extra_rows_lumping) against its byte model,
   and the added time per multigrid iteration (alternating lsq_iterate rounds of the two handles
   with precond 4; a V-cycle applies level 0 five times) against 5 × this run's k_xr_fwd + k_xr_atq.

Usage: python tools/prior_step.py OUT.json [--config c4] [--steps 200] [--rounds 5] [--no-solves] [--mg OUT_MG.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOL = dict(atol=1e-12, btol=1e-12, conlim=1e12)


def frame_rows(gd, ref, tile_nodes, strip_nodes):
    """CSR of the frame's prior rows on the dz grid gd (shape (y, x, t))"""
    ny, nx, nt = gd.shape
    a, b = (ny - tile_nodes) // 2, (nx - tile_nodes) // 2
    yy, xx = np.meshgrid(np.arange(a, a + tile_nodes), np.arange(b, b + tile_nodes), indexing='ij')
    edge = (yy - a < strip_nodes) | (a + tile_nodes - 1 - yy < strip_nodes) | (xx - b < strip_nodes) | \
        (b + tile_nodes - 1 - xx < strip_nodes)
    y, x = yy[edge], xx[edge]
    ts = np.array([t for t in range(nt) if t != ref])
    Y, T = np.meshgrid(y, ts, indexing='ij')
    X = np.meshgrid(x, ts, indexing='ij')[0]
    c1 = gd.col_0 + np.ravel_multi_index((Y.ravel(), X.ravel(), T.ravel()), gd.shape)
    c0 = gd.col_0 + np.ravel_multi_index((Y.ravel(), X.ravel(), np.full(T.size, ref)), gd.shape)
    n = c1.size
    cols = np.stack([c1, c0], axis=1).ravel().astype(np.int64)
    vals = np.tile([1., -1.], n)
    return np.arange(0, 2 * n + 1, 2, dtype=np.int64), cols, vals


def multigrid_leg(a, res, cases):
    """the priors inside the multigrid preconditioner (lumped into its coarse levels) at this size"""
    sys_plain, sys_prior = cases['plain'][0], cases['prior'][0]
    out = {k: res[k] for k in ('config', 'n_points', 'n_cols', 'tile_nodes', 'sigma', 'budget_rate_bytes_per_s')}
    out['extra_rows'] = res['extra_rows']
    ok, why = sys_prior.solver.cg_available(4)
    if not ok:
        raise RuntimeError(f'the multigrid does not carry the priors: {why}')
    out['levels'] = [list(map(int, lv)) for lv in sys_prior.solver.mg_info()[0]]
    out['lumping'] = sys_prior.solver.extra_rows_mg_info()
    lump = sys_prior.solver.profile_extra_rows_lumping(reps=20)
    out['lump_pass_us'] = 1e3 * lump['k_mg_lump_xr']
    out['lump1_us'] = 1e3 * lump['k_mg_lump1']
    out['lump_pass_budget_us'] = 1e6 * out['lumping']['pass_bytes'] / res['budget_rate_bytes_per_s']
    out['lump_pass_bytes_per_s'] = out['lumping']['pass_bytes'] / max(1e-3 * lump['k_mg_lump_xr'], 1e-12)
    # converged solves, cold starts
    out['solves'] = {}
    xs = {}
    for label, name, pc in (('block_jacobi_priors', 'prior', 3), ('multigrid_lumped_priors', 'prior', 4),
                            ('multigrid_no_priors', 'plain', 4)):
        fs, _, b = cases[name]
        runs = []
        for _ in range(3):
            xs[label], st = fs.solver.solve(b, precond=pc, method=1, maxit=200000, b_rows=fs.n_data, **TOL)
            runs.append({'iters': int(st['iters']), 'istop': int(st['istop']), 'time_s': float(st['time_s']),
                         'setup_s': float(st.get('setup_s', 0.))})
        best = min(runs, key=lambda r: r['time_s'])
        out['solves'][label] = dict(best, runs=runs)
        print(label, out['solves'][label], flush=True)
    xb, xm = xs['block_jacobi_priors'], xs['multigrid_lumped_priors']
    out['solution_rel_diff'] = float(np.linalg.norm(xm - xb) / np.linalg.norm(xb))
    # the step: alternating rounds of precond 4 iterations on the two handles
    t = {'plain': [], 'prior': []}
    for _ in range(a.rounds):
        for name in t:
            fs, _, b = cases[name]
            fs.solver.iterate(b, 8, precond=4, method=1, b_rows=fs.n_data)
            st = fs.solver.iterate(b, a.mg_steps, precond=4, method=1, b_rows=fs.n_data)
            t[name].append(1e3 * st['time_s'] / a.mg_steps)
    e = {'steps': a.mg_steps, 'step_ms_plain': float(np.median(t['plain'])), 'step_ms_prior': float(np.median(t['prior'])),
         'step_ms_plain_all': t['plain'], 'step_ms_prior_all': t['prior']}
    e['extra_us'] = 1e3 * (e['step_ms_prior'] - e['step_ms_plain'])
    if 'step' in res:   # level 0 is applied five times per iteration: the CG step, one pre-smoothing step, the
        k = res['step']['kernels_us']   # residual, two post-smoothing steps
        e['kernels_us'] = {n: k[n] for n in ('k_xr_fwd', 'k_xr_atq')}
        e['five_applications_us'] = 5. * (k['k_xr_fwd'] + k['k_xr_atq'])
    out['step'] = e
    print(e, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('--config', default='c4')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--tile-km', type=float, default=80.)
    ap.add_argument('--strip-km', type=float, default=3.)
    ap.add_argument('--no-solves', action='store_true')
    ap.add_argument('--mg', default=None, help='write the multigrid leg (lumped priors) to this file')
    ap.add_argument('--mg-steps', type=int, default=48)
    a = ap.parse_args()

    import lssurf_amd as LS
    from lssurf_amd import synthetic
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    from lssurf_amd.smooth_fit import FitSystem

    D, kw = synthetic.points(a.config)
    S = LS.smooth_fit(data=D, return_fit_objects=True, VERBOSE=False, **kw)
    gd = S['grids']['dz']
    keep = reference_epoch_keep_cols(S['G_data'].col_N, gd, kw['reference_epoch'])
    w = np.abs(1. / np.concatenate((S['Ed'], S['Ec'])))
    rhs = np.zeros(w.size)
    rhs[:S['data'].size] = S['data'].z
    dx = kw['spacing']['dz']
    tile_nodes = min(int(round(a.tile_km * 1e3 / dx)) + 1, min(gd.shape[:2]))
    csr = frame_rows(gd, kw['reference_epoch'], tile_nodes, int(round(a.strip_km * 1e3 / dx)))
    m_x = csr[0].size - 1
    wx = np.full(m_x, 1. / 0.1)
    prior = 0.05 * np.random.default_rng(1).standard_normal(m_x)
    sys_plain = FitSystem(S['G_data'], S['Gc'], keep, S['Gc'].col_N, grids=S['grids'])
    sys_prior = FitSystem(S['G_data'], S['Gc'], keep, S['Gc'].col_N, grids=S['grids'], extra_csr=csr,
                          extra_mg=a.mg is not None)
    cases = {'plain': (sys_plain, w, rhs), 'prior': (sys_prior, np.r_[w, wx], np.r_[rhs, prior])}
    res = {'config': a.config, 'n_points': int(sys_plain.n_data), 'n_cols': int(keep.size), 'steps': a.steps,
           'rounds': a.rounds, 'tile_nodes': tile_nodes, 'sigma': 0.1, 'timing': 'device events around the '
           'iterations (stats time_s), medians of alternating rounds in one process',
           'budget_rate_bytes_per_s': 0.43 * 8e12}
    try:
        for fs, ww, _ in cases.values():
            fs.solver.set_row_weight(ww)
            fs.solver.set_row_mask(np.ones(ww.size, bool))
        res['extra_rows'] = sys_prior.solver.extra_rows_info()

        def step(name):
            fs, _, b = cases[name]
            fs.solver.iterate(b, 32, precond=3, method=1, b_rows=fs.n_data)       # init + warm-up
            st = fs.solver.iterate(b, a.steps, precond=3, method=1, b_rows=fs.n_data)
            return 1e3 * st['time_s'] / a.steps, st['bytes_per_iter']

        t = {'plain': [], 'prior': []}
        by = {}
        for _ in range(a.rounds):
            for name in t:
                ms, by[name] = step(name)
                t[name].append(ms)
        e = {'step_ms_plain': float(np.median(t['plain'])), 'step_ms_prior': float(np.median(t['prior'])),
             'step_ms_plain_all': t['plain'], 'step_ms_prior_all': t['prior'],
             'it_per_s_plain': 1e3 / float(np.median(t['plain'])), 'it_per_s_prior': 1e3 / float(np.median(t['prior'])),
             'model_bytes': float(by['prior'] - by['plain']), 'bytes_per_iter_plain': float(by['plain'])}
        e['extra_us'] = 1e3 * (e['step_ms_prior'] - e['step_ms_plain'])
        e['budget_us'] = 1e6 * e['model_bytes'] / res['budget_rate_bytes_per_s']
        e['rows_share_of_step_bytes'] = e['model_bytes'] / float(by['prior'])
        # the kernels' own times, inside real iterations of the live state the rounds left behind
        fs = sys_prior
        fs.solver.iterate(cases['prior'][2], 32, precond=3, method=1, b_rows=fs.n_data)
        k = fs.solver.profile_extra_rows(reps=max(a.steps, 20), precond=3)
        info = res['extra_rows']
        kept = np.zeros(S['Gc'].col_N, bool)
        kept[keep] = True
        nnz = int(np.count_nonzero(kept[csr[1]]))   # the entries on removed (reference-epoch) columns are dropped
        fwd_bytes = 20. * nnz + 16. * info['m_x']                  # SELL entries with their p gathers, rs and t
        atq_bytes = 28. * nnz + 28. * info['touched_cols']         # transpose entries with rs and t, the columns' q
        e['kernels_us'] = {n: 1e3 * v for n, v in k.items()}
        e['kept_entries'] = nnz
        e['kernels_model_bytes'] = {'k_xr_fwd': fwd_bytes, 'k_xr_atq': atq_bytes}
        e['kernels_budget_us'] = {n: 1e6 * b / res['budget_rate_bytes_per_s']
                                  for n, b in e['kernels_model_bytes'].items()}
        e['kernels_bytes_per_s'] = {n: e['kernels_model_bytes'][n] / (1e-3 * k[n]) for n in e['kernels_model_bytes']}
        res['step'] = e
        print(e, flush=True)
        if not a.no_solves:
            res['solve_block_jacobi'] = {}
            for name, (fs, _, b) in cases.items():
                _, st = fs.solver.solve(b, precond=3, method=1, maxit=200000, b_rows=fs.n_data, **TOL)
                res['solve_block_jacobi'][name] = {'iters': int(st['iters']), 'istop': int(st['istop']),
                                                   'time_s': float(st['time_s'])}
                print(name, res['solve_block_jacobi'][name], flush=True)
        if a.mg:
            res_mg = multigrid_leg(a, res, cases)
    finally:
        sys_plain.close()
        sys_prior.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if a.mg:
        os.makedirs(os.path.dirname(os.path.abspath(a.mg)), exist_ok=True)
        with open(a.mg, 'w') as f:
            json.dump(res_mg, f, indent=1)
        print(json.dumps(res_mg))


if __name__ == '__main__':
    main()
