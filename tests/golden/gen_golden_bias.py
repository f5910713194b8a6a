#!/usr/bin/env python3
"""Generate tests/golden/sys_bias.npz and sys_bias_edit.npz: smooth_fit with data biases
(bias_params: one additive offset per unique (sensor, cycle) combination, bias_functions.py) run by
the REFERENCE, with the stand-ins of _refstubs.py and the helpers of gen_golden.py (a no-op where
the reference is absent).  The fixtures hold inputs and outputs only.

Both: the sekeys domain (1400 × 1200, 1 000 points, 100 m spacing, dt 0.25, reference_epoch 2,
4 outer iterations, outliers); fields sensor ∈ {0, 1, 2} and cycle ∈ 0 … 5 give 18 bias IDs;
sigma_corr is 0.01 for sensor 0 and 0.5 for the others, whose data carry true offsets ~N(0, 0.5).
sys_bias_edit gives one ID an offset of about 10 × its sigma_corr and sets bias_nsigma_edit = 3, so
the reference's edit_by_bias removes it.

The reference asks pointCollection for unique_by_rows; the stand-in module gets the reference's own
LSsurf.unique_by_rows here.  run_sf cannot store m['bias'] (it expects grid containers), so the
outputs are written here.

The tests allow no edit flip, so the seeds must leave no point of any outer iteration within 1e-6
of the editing threshold |r / sigma_aug| = 3: every sigma_extra the reference computes is recorded
and the margin asserted here, on the CPU.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import E_RMS_NB, _csr_arrays, synth_points   # noqa: E402

SEEDS = {'bias': 20261101, 'bias_edit': 20261102}
BIAS_PARAMS = ['sensor', 'cycle']


def gen_bias(LS, stubs, name, edit):
    import pointCollection as pc
    from oracle import dense
    rng = np.random.default_rng(SEEDS[name])
    W = {'x': 1400., 'y': 1200., 't': 1.25}
    ctr = {'x': 0., 'y': 0., 't': 0.}
    x, y, t, z = synth_points(rng, W, ctr, 1000)
    sensor = rng.integers(0, 3, x.size).astype(float)
    cycle = rng.integers(0, 6, x.size).astype(float)
    sigma_corr = np.where(sensor == 0, 0.01, 0.5)
    offset = rng.normal(0, 0.5, (3, 6))
    offset[0] = 0.
    big = (1, 3)            # (sensor, cycle) of the ID the edit fixture pushes out
    if edit:
        offset[big] = 5.0   # 10 × its sigma_corr
    z = z + offset[sensor.astype(int), cycle.astype(int)]
    bad = rng.random(x.size) > 0.93
    z[bad] += (rng.random(bad.sum()) - 0.5) * 40
    data_dict = {'x': x, 'y': y, 'time': t, 'z': z, 'sigma': np.full(x.size, 0.1), 'sensor': sensor,
                 'cycle': cycle, 'sigma_corr': sigma_corr}
    kw = dict(W=W, ctr=ctr, spacing={'z0': 100., 'dz': 100., 'dt': 0.25}, E_RMS=E_RMS_NB, reference_epoch=2,
              max_iterations=4, VERBOSE=False, dzdt_lags=[1], bias_params=list(BIAS_PARAMS))
    if edit:
        kw['bias_nsigma_edit'] = 3

    # record every sigma_extra the reference computes, to measure the editing margin
    sf_mod = sys.modules['LSsurf.smooth_fit']
    ref_se = sf_mod.calc_sigma_extra
    calls = []

    def recording(r, sigma, in_TSE, *a, **k):
        se = ref_se(r, sigma, in_TSE, *a, **k)
        calls.append((np.array(r), np.array(sigma), np.array(se)))
        return se

    # the reference does not return its bias model: keep the dict its assign_bias_ID hands to the fit
    # (edit_by_bias marks the edited IDs in it, in place)
    ref_assign = sf_mod.assign_bias_ID
    models = []

    def keeping(*a, **k):
        d, bm = ref_assign(*a, **k)
        models.append(bm)
        return d, bm

    sf_mod.calc_sigma_extra = recording
    sf_mod.assign_bias_ID = keeping
    stubs.CALLS.clear()
    stubs.SOLS.clear()
    try:
        S = LS.smooth_fit(data=pc.data().from_dict(data_dict), **kw)
    finally:
        sf_mod.calc_sigma_extra = ref_se
        sf_mod.assign_bias_ID = ref_assign
    assert len(models) == 1
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
    for f in ['z_est', 'three_sigma_edit', 'sigma_extra', 'bias_ID']:
        out['data_' + f] = np.asarray(getattr(d, f))
    out['valid_data'] = np.asarray(S['valid_data'])
    bias = m['bias']
    for k in ['val', 'ID', 'expected', 'rms_data_raw', 'rms_data_edited', 'N_raw', 'N_edited'] + BIAS_PARAMS:
        out['bias_' + k] = np.asarray(bias[k], dtype=float)
    out['bias_keys'] = np.array(list(bias.keys()))
    out['kwargs'] = np.array(repr(kw))
    n_id = out['bias_ID'].size
    # the IDs the reference's edit_by_bias removed: its own flags, in the order of bias_param_dict['ID']
    pd = models[0]['bias_param_dict']
    assert list(pd['ID']) == [int(j) for j in out['bias_ID']]
    edited = np.array(pd['edited'], dtype=bool) if 'edited' in pd else np.zeros(n_id, dtype=bool)
    out['bias_edited'] = edited
    for j in out['bias_ID'][edited]:   # their data are all out, so their bias is 0
        assert not np.any((out['data_bias_ID'] == j) & (out['data_three_sigma_edit'] == 1))
    assert n_id == 18, n_id
    if edit:
        assert edited.any() and not edited.all(), 'the reference must edit at least one ID and keep at least one'
    np.savez_compressed(os.path.join(HERE, f'sys_{name}.npz'), **out)
    print(f'{name}: A {A.shape} nnz {A.nnz}, solves {len(stubs.CALLS)}, opt {float(out["x_opt"]):.2e}, {n_id} IDs, '
          f'{int(edited.sum())} edited, editing margin {margin:.3e}')


def main():
    import _refstubs
    if not os.path.isdir(_refstubs.REF):
        print('gen_golden_bias: reference absent; keeping the committed fixtures')
        return
    LS = _refstubs.install()
    from LSsurf.unique_by_rows import unique_by_rows
    sys.modules['pointCollection'].unique_by_rows = unique_by_rows
    gen_bias(LS, _refstubs, 'bias', False)
    gen_bias(LS, _refstubs, 'bias_edit', True)


if __name__ == '__main__':
    main()
