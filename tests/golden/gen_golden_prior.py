#!/usr/bin/env python3
"""Generate tests/golden/sys_prior_edge.npz and sys_prior_dz.npz: smooth_fit with the tile-edge
priors (prior_edge_args, match_priors.match_tile_edges) and with a dz prior (prior_args,
match_priors.match_prior_dz) run by the REFERENCE, with the stand-ins of _refstubs.py and the
helpers of gen_golden.py (a no-op where the reference is absent).  The fixtures hold inputs and
outputs only: data, tiles, A, b, x, z0, dz, data_*, valid_data, kwargs.

Domain (both): a square tile of 1 600 m centred on (0, 0) at 100 m spacing, dt 0.25 over 1.25 yr,
reference_epoch 2 (t = −0.125), 1 000 points, 4 outer iterations with outliers.

sys_prior_edge: tile_spacing 1 000, edge_include 300.  The stand-in pointCollection.grid.data gets a
from_h5 / as_points of its own here, at run time and in this generator only: from_h5 returns the
in-memory neighbour tile keyed by the file's base name, and prior_dir is a temporary directory of
empty E*_N*.h5 files, so the reference's match_tile_edges and make_prior_op run unmodified.  Four
neighbour tiles and the tile itself: E1_N0, E0_N1, E-1_N0 (used; tile_names records the order of the reference's
glob), E3_N0 (too far: skipped), E0_N0 (the fit's own centre: skipped).  Their nodes are 130 m apart on a lattice shifted against the
fit's, their epochs (−0.5, −0.3, −0.125, 0.1, 0.45) fall between the fit's except the third, the
reference time, whose points must drop out; sigma_dz varies over 0.05 … 0.5.

sys_prior_dz: the reference's match_prior_dz cannot take an in-memory grid (its isinstance test
against a list raises TypeError), so it is patched here to a function that calls the reference's
make_prior_op on the grid's nodes as points.  The saved grid lies inside the fit's bounds on uniform,
binary-exact coordinates (epochs −0.5, −0.3125, −0.125, 0.0625, 0.25), so the reference's selection
for skip 1 / edge_pad 0 (its bounds are centre ± half-width) is every node.

The tests allow no edit flip: the editing margin (> 1e-6 from |r / sigma_aug| = 3) is asserted
here on every sigma_extra the reference computes.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import E_RMS_NB, _csr_arrays, synth_points   # noqa: E402

SEEDS = {'prior_edge': 20261201, 'prior_dz': 20261202}
TILE_T = np.array([-0.5, -0.3, -0.125, 0.1, 0.45])


def make_tile(rng, xc, yc, half=780., step=130., t=TILE_T):
    """a neighbour tile's saved dz grid: dz (y, x, t), smooth plus noise; sigma_dz 0.05 … 0.5"""
    x = xc + np.arange(-half, half + 1, step)
    y = yc + np.arange(-half, half + 1, step)
    yy, xx, tt = np.meshgrid(y, x, t, indexing='ij')
    dz = 0.5 * (tt - t[2]) * np.exp(-(xx ** 2 + yy ** 2) / 400. ** 2) + rng.normal(0, 0.02, yy.shape)
    sigma = 0.05 + 0.45 * rng.random(yy.shape)
    return {'x': x, 'y': y, 't': np.array(t), 'dz': dz, 'sigma_dz': sigma}


def grid_points(pc, g):
    """the nodes of a (y, x, t) grid dict as points, raveled in (y, x, t) order"""
    yy, xx, tt = np.meshgrid(g['y'], g['x'], g['t'], indexing='ij')
    return pc.data().from_dict({'x': xx.ravel(), 'y': yy.ravel(), 't': tt.ravel(), 'dz': g['dz'].ravel(),
                                'sigma_dz': g['sigma_dz'].ravel()})


def run(LS, stubs, name, kw, data_dict, extra):
    import pointCollection as pc
    from oracle import dense
    sf_mod = sys.modules['LSsurf.smooth_fit']
    ref_se = sf_mod.calc_sigma_extra
    calls = []

    def recording(r, sigma, in_TSE, *a, **k):
        se = ref_se(r, sigma, in_TSE, *a, **k)
        calls.append((np.array(r), np.array(sigma), np.array(se)))
        return se

    sf_mod.calc_sigma_extra = recording
    stubs.CALLS.clear()
    stubs.SOLS.clear()
    try:
        S = LS.smooth_fit(data=pc.data().from_dict(data_dict), **kw)
    finally:
        sf_mod.calc_sigma_extra = ref_se
    assert calls, 'the reference never computed sigma_extra'
    margin = min(float(np.min(np.abs(np.abs(r / np.sqrt(s ** 2 + se ** 2)) - 3.0))) for r, s, se in calls)
    assert margin > 1e-6, f'{name}: a point sits on the editing threshold ({margin:.2e}): choose another seed'
    out = {'in_' + k: np.asarray(v) for k, v in data_dict.items()}
    A, b = stubs.CALLS[0]
    out.update(_csr_arrays('A', A))
    out['b'] = b
    out['x'] = stubs.SOLS[0]
    out['x_opt'] = np.array(dense.optimality(A, b, stubs.SOLS[0]))
    out['n_solves'] = np.array(len(stubs.CALLS))
    m, d = S['m'], S['data']
    out['z0'] = m['z0'].z0
    out['dz'] = m['dz'].dz
    out['m_all'] = m['all']
    for f in ['z_est', 'three_sigma_edit', 'sigma_extra']:
        out['data_' + f] = np.asarray(getattr(d, f))
    out['valid_data'] = np.asarray(S['valid_data'])
    out['n_data'] = np.array(d.size)
    out['n_prior'] = np.array(sum(len(S['TOC']['rows'][k]) for k in S['TOC']['rows'] if k.startswith('prior_dz1_')))
    out.update({k: (v() if callable(v) else v) for k, v in extra.items()})
    np.savez_compressed(os.path.join(HERE, f'sys_{name}.npz'), **out)
    print(f'{name}: A {A.shape} nnz {A.nnz}, solves {len(stubs.CALLS)}, opt {float(out["x_opt"]):.2e}, '
          f'{int(out["n_prior"])} prior rows, editing margin {margin:.3e}')


def base_case(rng):
    W = {'x': 1600., 'y': 1600., 't': 1.25}
    ctr = {'x': 0., 'y': 0., 't': 0.}
    x, y, t, z = synth_points(rng, W, ctr, 1000)
    bad = rng.random(x.size) > 0.93
    z[bad] += (rng.random(bad.sum()) - 0.5) * 40
    data_dict = {'x': x, 'y': y, 'time': t, 'z': z, 'sigma': np.full(x.size, 0.1)}
    kw = dict(W=W, ctr=ctr, spacing={'z0': 100., 'dz': 100., 'dt': 0.25}, E_RMS=E_RMS_NB, reference_epoch=2,
              max_iterations=4, VERBOSE=False, dzdt_lags=[1])
    return data_dict, kw


def gen_edge(LS, stubs):
    import pointCollection as pc
    rng = np.random.default_rng(SEEDS['prior_edge'])
    data_dict, kw = base_case(rng)
    tiles = {'E1_N0': make_tile(rng, 1000., 0.), 'E0_N1': make_tile(rng, 0., 1000.),
             'E-1_N0': make_tile(rng, -1000., 0.), 'E3_N0': make_tile(rng, 3000., 0.),
             'E0_N0': make_tile(rng, 0., 0.)}
    G = pc.grid.data
    opened = []

    def from_h5(self, file, group=None, fields=None):
        key = os.path.basename(file)[:-3]
        opened.append(key)
        self.from_dict(tiles[key])
        self.filename = file
        return self

    def as_points(self):
        return grid_points(pc, {k: getattr(self, k) for k in ('x', 'y', 't', 'dz', 'sigma_dz')})

    G.from_h5, G.as_points = from_h5, as_points
    try:
        with tempfile.TemporaryDirectory() as d:
            for key in tiles:
                open(os.path.join(d, key + '.h5'), 'w').close()
            kw_run = dict(kw, prior_edge_args={'prior_dir': d, 'tile_spacing': 1000., 'edge_include': 300.})
            extra = {'kwargs': np.array(repr(dict(kw, prior_edge_args={'tile_spacing': 1000., 'edge_include': 300.}))),
                     # the order the reference read them in (its glob), then the two it skipped
                     'tile_names': lambda: np.array(opened + sorted(set(tiles) - set(opened)))}
            for key, g in tiles.items():
                for f, v in g.items():
                    extra[f'tile_{key}_{f}'] = v
            run(LS, stubs, 'prior_edge', kw_run, data_dict, extra)
    finally:
        del G.from_h5, G.as_points
    assert sorted(opened) == ['E-1_N0', 'E0_N1', 'E1_N0'], opened   # the far tile and the tile itself are skipped


def gen_dz(LS, stubs):
    import pointCollection as pc
    from LSsurf.match_priors import make_prior_op
    rng = np.random.default_rng(SEEDS['prior_dz'])
    data_dict, kw = base_case(rng)
    # inside the fit's bounds, off its lattice; uniform, binary-exact coordinates, so the reference's
    # centre ± half-width bounds (match_priors.py:85-92) are the grid's own ends
    g = make_tile(rng, 35., -20., half=650., t=-0.125 + 0.1875 * np.arange(-2, 3))
    sf_mod = sys.modules['LSsurf.smooth_fit']
    ref_mp = sf_mod.match_prior_dz

    def match_prior_dz(grids, dzs=None, ref_epoch=0, sigma_scale=1, **_):
        # the reference's in-memory branch raises TypeError (isinstance(datasrc, [pc.grid.data])):
        # its selection for skip 1 / edge_pad 0 is every node inside the grid's bounds
        out = []
        for d in dzs:
            bds = grids['dz'].bds
            assert d['y'][0] >= bds[0][0] and d['y'][-1] <= bds[0][1] and d['x'][0] >= bds[1][0] and \
                d['x'][-1] <= bds[1][1] and d['t'][0] >= bds[2][0] and d['t'][-1] <= bds[2][1]
            out.append(make_prior_op(grids, grid_points(pc, d), 'internal_prior', ref_time=d['t'][ref_epoch],
                                     sigma_scale=sigma_scale))
        return out

    sf_mod.match_prior_dz = match_prior_dz
    try:
        extra = {'kwargs': np.array(repr(dict(kw, prior_args={'ref_epoch': 2, 'sigma_scale': 2.}))),
                 'tile_names': np.array(['prior'])}
        for f, v in g.items():
            extra[f'tile_prior_{f}'] = v
        run(LS, stubs, 'prior_dz', dict(kw, prior_args={'dzs': [g], 'ref_epoch': 2, 'sigma_scale': 2.}), data_dict,
            extra)
    finally:
        sf_mod.match_prior_dz = ref_mp


def main():
    import _refstubs
    if not os.path.isdir(_refstubs.REF):
        print('gen_golden_prior: reference absent; keeping the committed fixtures')
        return
    LS = _refstubs.install()
    gen_edge(LS, _refstubs)
    gen_dz(LS, _refstubs)


if __name__ == '__main__':
    main()
