#!/usr/bin/env python3
"""Generate tests/golden/sys_slope.npz: smooth_fit with data biases and slope biases
(data_slope_sensors: one tilt in x and one in y per listed sensor, data_slope_bias.py) run by the
REFERENCE, with the stand-ins of _refstubs.py and the helpers of gen_golden.py (a no-op where the
reference is absent).  The fixture holds inputs and outputs only.

The bias fixture's domain (1400 × 1200, 1 000 points, 100 m spacing, dt 0.25, reference_epoch 2,
4 outer iterations, outliers); fields sensor ∈ {0, 1, 2, 3} and cycle ∈ 0 … 5 give 24 bias IDs;
sigma_corr is 0.01 for sensor 0 and 0.5 for the others, whose data carry true offsets ~N(0, 0.5).
The data of sensors 1 and 2 also carry true tilts ~N(0, 0.005) m/m in x and in y.
data_slope_sensors = [1, 2, 7]: sensor 7 is absent and the reference filters it out, so the model
gains 4 slope columns behind the 24 bias columns.

As in gen_golden_bias.py the tests allow no edit flip, so the seed must leave no point of any outer
iteration within 1e-6 of the editing threshold |r / sigma_aug| = 3: every sigma_extra the reference
computes is recorded and the margin asserted here, on the CPU.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import E_RMS_NB, _csr_arrays, synth_points   # noqa: E402

SEED = 20261201
BIAS_PARAMS = ['sensor', 'cycle']
SLOPE_SENSORS = [1., 2., 7.]


def gen_slope(LS, stubs):
    import pointCollection as pc
    from oracle import dense
    rng = np.random.default_rng(SEED)
    W = {'x': 1400., 'y': 1200., 't': 1.25}
    ctr = {'x': 0., 'y': 0., 't': 0.}
    x, y, t, z = synth_points(rng, W, ctr, 1000)
    sensor = rng.integers(0, 4, x.size).astype(float)
    cycle = rng.integers(0, 6, x.size).astype(float)
    sigma_corr = np.where(sensor == 0, 0.01, 0.5)
    offset = rng.normal(0, 0.5, (4, 6))
    offset[0] = 0.
    tilt = np.zeros((4, 2))
    tilt[1:3] = rng.normal(0, 0.005, (2, 2))   # m/m, sensors 1 and 2
    z = z + offset[sensor.astype(int), cycle.astype(int)]
    for s in (1, 2):
        mine = sensor == s
        z[mine] += tilt[s, 0] * (x[mine] - x[mine].mean()) + tilt[s, 1] * (y[mine] - y[mine].mean())
    bad = rng.random(x.size) > 0.93
    z[bad] += (rng.random(bad.sum()) - 0.5) * 40
    data_dict = {'x': x, 'y': y, 'time': t, 'z': z, 'sigma': np.full(x.size, 0.1), 'sensor': sensor,
                 'cycle': cycle, 'sigma_corr': sigma_corr}
    kw = dict(W=W, ctr=ctr, spacing={'z0': 100., 'dz': 100., 'dt': 0.25}, E_RMS=E_RMS_NB, reference_epoch=2,
              max_iterations=4, VERBOSE=False, dzdt_lags=[1], bias_params=list(BIAS_PARAMS),
              data_slope_sensors=list(SLOPE_SENSORS))   # recorded as a list; the fit gets an array

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
        # the reference indexes data_slope_sensors as an array
        S = LS.smooth_fit(data=pc.data().from_dict(data_dict),
                          **{**kw, 'data_slope_sensors': np.array(SLOPE_SENSORS)})
    finally:
        sf_mod.calc_sigma_extra = ref_se
    assert calls, 'the reference never computed sigma_extra'
    margin = min(float(np.min(np.abs(np.abs(r / np.sqrt(s ** 2 + se ** 2)) - 3.0))) for r, s, se in calls)
    assert margin > 1e-6, f'slope: a point sits on the editing threshold ({margin:.2e}): choose another seed'

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
    # the slopes: the sensors the reference kept, and (slope_x, slope_y) of each, in m/km
    slope = m['slope_bias']
    out['slope_keys'] = np.array([float(k) for k in slope.keys()])
    out['slope_val'] = np.array([[slope[k]['slope_x'], slope[k]['slope_y']] for k in slope.keys()], dtype=float)
    out['slope_true'] = 1000. * tilt[1:3]
    out['kwargs'] = np.array(repr(kw))
    n_id, n_slope = out['bias_ID'].size, out['slope_val'].size
    assert n_id == 24, n_id
    assert n_slope == 4 and list(out['slope_keys']) == [1., 2.], out['slope_keys']
    assert A.shape[1] == out['x'].size and np.array_equal(out['m_all'][-4:], out['slope_val'].ravel())
    np.savez_compressed(os.path.join(HERE, 'sys_slope.npz'), **out)
    print(f'slope: A {A.shape} nnz {A.nnz}, solves {len(stubs.CALLS)}, opt {float(out["x_opt"]):.2e}, {n_id} IDs, '
          f'slopes {out["slope_val"].ravel()} (true {out["slope_true"].ravel()}), editing margin {margin:.3e}')


def main():
    import _refstubs
    if not os.path.isdir(_refstubs.REF):
        print('gen_golden_slope: reference absent; keeping the committed fixture')
        return
    LS = _refstubs.install()
    from LSsurf.unique_by_rows import unique_by_rows
    sys.modules['pointCollection'].unique_by_rows = unique_by_rows
    gen_slope(LS, _refstubs)


if __name__ == '__main__':
    main()
