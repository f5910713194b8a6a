#!/usr/bin/env python3
"""Generate tests/golden/sys_bias_E.npz: the uncertainties of the sys_bias configuration
(gen_golden_bias.py; the inputs and keywords are read back from sys_bias.npz) as the REFERENCE's
smooth_fit(compute_E=True) reports them, with the stand-ins of _refstubs.py (a no-op where the
reference is absent).  The fixture holds outputs only:

* Eref_sigma_z0, Eref_sigma_dz, Eref_sigma_bias: E['sigma_z0'], E['sigma_dz'] and
  E['sigma_bias']['val'] of the reference (its inv_tr_upper drops |R⁻¹| ≤ 1e-5);
* Eexact_*: the same from an exact inverse, sqrt(diag((AᵀA)⁻¹)) of the matrix the reference handed
  to sparseqr.rz, laid out through the reference's own Ip_c and table of contents;
* trunc_rel_diff: the largest difference between the two sets, relative to each grid's maximum —
  the reference's own truncation error, which the test allows ten times over.
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def main():
    import _refstubs
    if not os.path.isdir(_refstubs.REF):
        print('gen_golden_bias_E: reference absent; keeping the committed fixture')
        return
    LS = _refstubs.install()
    import pointCollection as pc
    from LSsurf.unique_by_rows import unique_by_rows
    from LSsurf.constraint_functions import build_reference_epoch_matrix
    sys.modules['pointCollection'].unique_by_rows = unique_by_rows
    g = np.load(os.path.join(HERE, 'sys_bias.npz'), allow_pickle=False)
    kw = ast.literal_eval(str(g['kwargs']))
    pts = {k[3:]: g[k] for k in g.files if k.startswith('in_')}

    # the reference's fit objects do not leave smooth_fit with compute_E: keep Ip_c's arguments
    sf_mod = sys.modules['LSsurf.smooth_fit']
    ref_build = sf_mod.build_reference_epoch_matrix
    seen = []

    def keeping(G_data, Gc, grids, ref_epoch):
        Ip_c = ref_build(G_data, Gc, grids, ref_epoch)
        seen.append((Ip_c, Gc.TOC))
        return Ip_c
    sf_mod.build_reference_epoch_matrix = keeping
    _refstubs.RZ_CALLS.clear()
    try:
        S = LS.smooth_fit(data=pc.data().from_dict(pts), compute_E=True, **kw)
    finally:
        sf_mod.build_reference_epoch_matrix = ref_build
    assert build_reference_epoch_matrix is ref_build and seen and len(_refstubs.RZ_CALLS) == 1
    E = S['E']
    ref = {'sigma_z0': np.asarray(E['sigma_z0'].sigma_z0), 'sigma_dz': np.asarray(E['sigma_dz'].sigma_dz),
           'sigma_bias': np.asarray(E['sigma_bias']['val'], dtype=float)}
    assert np.array_equal(np.asarray(E['sigma_bias']['ID'], dtype=float), g['bias_ID'])
    assert not E['sigma_slope_bias']

    A = _refstubs.RZ_CALLS[0]
    Ip_c, TOC = seen[-1]
    E0 = Ip_c.dot(np.sqrt(np.diag(np.linalg.inv((A.T @ A).toarray()))))
    bias_cols = np.arange(ref['sigma_z0'].size + ref['sigma_dz'].size, E0.size)
    assert bias_cols.size == ref['sigma_bias'].size
    exact = {'sigma_z0': E0[TOC['cols']['z0']].reshape(ref['sigma_z0'].shape),
             'sigma_dz': E0[TOC['cols']['dz']].reshape(ref['sigma_dz'].shape), 'sigma_bias': E0[bias_cols]}
    out, trunc = {}, 0.
    for k in ref:
        out['Eref_' + k], out['Eexact_' + k] = ref[k], exact[k]
        trunc = max(trunc, float(np.abs(ref[k] - exact[k]).max() / np.abs(exact[k]).max()))
    out['trunc_rel_diff'] = np.array(trunc)
    np.savez_compressed(os.path.join(HERE, 'sys_bias_E.npz'), **out)
    print(f"bias_E: {A.shape[1]} columns, {bias_cols.size} biases, the reference's truncation moves sigma by {trunc:.2e}")


if __name__ == '__main__':
    main()
