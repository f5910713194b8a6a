#!/usr/bin/env python3
"""Generate tests/golden/sys_sgrid_joint.npz: smooth_fit with data biases, slope biases and sensor
bias grids together (bias_params, data_slope_sensors, sensor_grid_bias_params) run by the REFERENCE,
with the stand-ins of _refstubs.py and the helpers of gen_golden.py (a no-op where the reference is
absent).  The fixture holds inputs and outputs only.

The slope fixture's domain (1400 × 1200, 1 000 points, 100 m spacing, dt 0.25, reference_epoch 2,
4 outer iterations, 7 % outliers of ± 20 m); sensor ∈ 0 … 4 and cycle ∈ 0 … 5 give 30 bias IDs;
sigma_corr is 0.01 for sensor 0 and 0.5 for the others, whose data carry true offsets ~N(0, 0.5).
Sensors 1, 2 and 3 carry true tilts ~N(0, 0.005) m/m, sensors 1, 2 and 4 the warp of gen_golden_sgrid.py.
Every case of the joint elimination at once: sensor 0 has loose biases only; sensors 1 and 2 biases,
slopes and a grid (sensor 2's with a magnitude prior); sensor 3 biases and slopes without a grid;
sensor 4 biases and a grid without slopes; sensor 7 is absent from both lists' data.

The tests allow no edit flip, so the seed must leave no point of any outer iteration within 1e-6 of
the editing threshold |r / sigma_aug| = 3: every sigma_extra the reference computes is recorded and
the margin asserted here, on the CPU.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import E_RMS_NB, _csr_arrays, synth_points   # noqa: E402

SEED = 20280101
BIAS_PARAMS = ['sensor', 'cycle']
SLOPE_SENSORS = [1., 2., 3., 7.]
GRID_PARAMS = [{'sensor': 1., 'spacing': 200., 'expected_rms': 1.0, 'expected_rms_grad2': 1e-5},
               {'sensor': 2., 'spacing': 300., 'expected_rms': 0.5, 'expected_val': 0.25},
               {'sensor': 4., 'spacing': 300., 'expected_rms': 0.5},
               {'sensor': 7., 'spacing': 200., 'expected_rms': 1.0}]


def gen_sgrid_joint(LS, stubs):
    import pointCollection as pc
    from oracle import dense
    rng = np.random.default_rng(SEED)
    W = {'x': 1400., 'y': 1200., 't': 1.25}
    ctr = {'x': 0., 'y': 0., 't': 0.}
    x, y, t, z = synth_points(rng, W, ctr, 1000)
    sensor = rng.integers(0, 5, x.size).astype(float)
    cycle = rng.integers(0, 6, x.size).astype(float)
    sigma_corr = np.where(sensor == 0, 0.01, 0.5)
    offset = rng.normal(0, 0.5, (5, 6))
    offset[0] = 0.
    tilt = np.zeros((5, 2))
    tilt[1:4] = rng.normal(0, 0.005, (3, 2))   # m/m, sensors 1, 2 and 3
    z = z + offset[sensor.astype(int), cycle.astype(int)]
    for s in (1, 2, 3):
        mine = sensor == s
        z[mine] += tilt[s, 0] * (x[mine] - x[mine].mean()) + tilt[s, 1] * (y[mine] - y[mine].mean())
    warp = 0.8 * np.sin(2 * np.pi * x / 900.) * np.cos(2 * np.pi * y / 700.)
    z = z + np.where((sensor == 1) | (sensor == 2) | (sensor == 4), warp, 0.)
    bad = rng.random(x.size) > 0.93
    z[bad] += (rng.random(bad.sum()) - 0.5) * 40
    data_dict = {'x': x, 'y': y, 'time': t, 'z': z, 'sigma': np.full(x.size, 0.1), 'sensor': sensor,
                 'cycle': cycle, 'sigma_corr': sigma_corr}
    kw = dict(W=W, ctr=ctr, spacing={'z0': 100., 'dz': 100., 'dt': 0.25}, E_RMS=E_RMS_NB, reference_epoch=2,
              max_iterations=4, VERBOSE=False, dzdt_lags=[1], bias_params=list(BIAS_PARAMS),
              data_slope_sensors=list(SLOPE_SENSORS),   # recorded as a list; the fit gets an array
              sensor_grid_bias_params=[dict(p) for p in GRID_PARAMS])

    # record every sigma_extra the reference computes, to measure the editing margin
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
        S = LS.smooth_fit(data=pc.data().from_dict(data_dict),
                          **{**kw, 'data_slope_sensors': np.array(SLOPE_SENSORS),
                             'sensor_grid_bias_params': [dict(p) for p in GRID_PARAMS]})
    finally:
        sf_mod.calc_sigma_extra = ref_se
    assert calls, 'the reference never computed sigma_extra'
    margin = min(float(np.min(np.abs(np.abs(r / np.sqrt(s ** 2 + se ** 2)) - 3.0))) for r, s, se in calls)
    assert margin > 1e-6, f'sgrid_joint: a point sits on the editing threshold ({margin:.2e}): choose another seed'

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
    for f in ['z_est', 'three_sigma_edit', 'sigma_extra', 'bias_ID']:
        out['data_' + f] = np.asarray(getattr(d, f))
    out['valid_data'] = np.asarray(S['valid_data'])
    bias = m['bias']
    for k in ['val', 'ID', 'expected', 'rms_data_raw', 'rms_data_edited', 'N_raw', 'N_edited'] + BIAS_PARAMS:
        out['bias_' + k] = np.asarray(bias[k], dtype=float)
    out['bias_keys'] = np.array(list(bias.keys()))
    out['bias_edited'] = np.zeros(out['bias_ID'].size, dtype=bool)
    slope = m['slope_bias']
    out['slope_keys'] = np.array([float(k) for k in slope.keys()])
    out['slope_val'] = np.array([[slope[k]['slope_x'], slope[k]['slope_y']] for k in slope.keys()], dtype=float)
    out['slope_true'] = 1000. * tilt[1:4]
    sg = m['sensor_bias_grids']
    out['sgrid_keys'] = np.array(list(sg.keys()))
    for k, name in enumerate(sg.keys()):
        for f in ('x', 'y', 'z'):
            out[f'sgrid{k}_{f}'] = np.asarray(getattr(sg[name], f), dtype=float)
    out['kwargs'] = np.array(repr(kw))
    shapes = [tuple(out[f'sgrid{k}_z'].shape) for k in range(len(sg))]
    n_sg = sum(int(np.prod(s)) for s in shapes)
    n_id, n_slope = out['bias_ID'].size, out['slope_val'].size
    assert list(sg.keys()) == ['sensor_1.0_bias', 'sensor_2.0_bias', 'sensor_4.0_bias'], list(sg.keys())
    assert n_id == 30 and n_slope == 6 and list(out['slope_keys']) == [1., 2., 3.], (n_id, out['slope_keys'])
    assert A.shape[1] == out['x'].size
    # the reference's column order: z0, dz, the biases, the slopes, the sensor grids
    assert np.array_equal(out['m_all'][-n_sg:], np.concatenate([out[f'sgrid{k}_z'].ravel() for k in range(len(sg))]))
    assert np.array_equal(out['m_all'][-n_sg - n_slope:-n_sg], out['slope_val'].ravel())
    np.savez_compressed(os.path.join(HERE, 'sys_sgrid_joint.npz'), **out)
    print(f'sgrid_joint: A {A.shape} nnz {A.nnz}, solves {len(stubs.CALLS)}, opt {float(out["x_opt"]):.2e}, '
          f'grids {shapes}, {n_id} IDs, slopes of sensors {list(out["slope_keys"])}, '
          f'{int(np.sum(~out["data_three_sigma_edit"].astype(bool)))} points edited, editing margin {margin:.3e}')


def main():
    import _refstubs
    if not os.path.isdir(_refstubs.REF):
        print('gen_golden_sgrid_joint: reference absent; keeping the committed fixture')
        return
    LS = _refstubs.install()
    from LSsurf.unique_by_rows import unique_by_rows
    sys.modules['pointCollection'].unique_by_rows = unique_by_rows
    gen_sgrid_joint(LS, _refstubs)


if __name__ == '__main__':
    main()
