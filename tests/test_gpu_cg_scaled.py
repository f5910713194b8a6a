"""Per-row constraint scales inside CGNR: lsq_set_cg_scaled, FitSystem(cg_scaled=True),
smooth_fit(lsq_cg_scaled=True); k_cg_scaled in lssurf_amd/csrc/lsqr_cg.inc.

A mask with mask_scale, or constraint_scaling_maps, gives the constraint rows one row scale per (y, x) node.
Without the key the device has no class-table normal stencil for such a part: lsq_cg_available is 0 ("a
stencil part has per-row scales …") and method 1 falls back to LSQR.  With it the part leaves the class
table and k_cg_scaled applies it from a squared-scale field.  The systems, the expected part counts and the
exact solutions are those of tests/scaled_host.py (pinned on the host by tests/test_scaled_host.py).

Bounds: the operator against Aᵀ(A p) of get_csr() within 1e-12 of max |AᵀA p| (the suite's operator bound);
converged solves (atol = btol = 1e-12) against the exact solution within DESIGN.md's REL 1e-6 / ABS 1e-4; the
iterates within τ_k = max(1000·e_k, 1e-13) of cgnr_host.pcg in extended precision, the rule of
tests/test_gpu_cgnr_iterates.py.  Device solves run before get_csr(), as that file explains."""
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import conftest  # noqa: F401
import cgnr_host as H
import scaled_host as SH
import lssurf_amd as LS
from lssurf_amd import synthetic
from lssurf_amd._native import NativeError
from oracle.dense import ls_solve_dense
from test_gpu_cgnr import ABS, REL, TOL as TIGHT
from test_gpu_cgnr_iterates import Ref, _blocks, _check_iterates, _same_as_host, _solves

pytestmark = pytest.mark.gpu
NAMES = list(SH.SYSTEMS)
OP_TOL = 1e-12   # the suite's operator bound


def _open(h, w=None, mask=None, scaled=True, **kw):
    """a handle with the key (or without), the weights and mask set; no question asked of it yet"""
    fs = h.fit_system(cg_scaled=True, **kw) if scaled else h.fit_system(**kw)
    try:
        assert fs.formation == 'stencil' and fs.has_blocks
        fs.solver.set_row_weight(h.w if w is None else w)
        fs.solver.set_row_mask(np.ones(fs.n_data + fs.n_con, bool) if mask is None else mask)
    except BaseException:
        fs.close()
        raise
    return fs


def _full(fs, p):
    pf = np.zeros(fs.n_full)
    pf[fs.keep_cols] = p
    return pf


def _close(x, ref, tag):
    rel = np.linalg.norm(x - ref) / np.linalg.norm(ref)
    mx = float(np.max(np.abs(x - ref)))
    print(f'{tag}: rel {rel:.2e}, max {mx:.2e}')
    assert rel <= REL and mx <= ABS, (tag, rel, mx)


# ---- 1. operator -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operator(name):
    """availability, the scaled-part count, N p on two random p with 20 % of the data rows masked (twice:
    run to run), and get_csr() last"""
    h = SH.host(name)
    mask = SH.data_mask(h)
    rng = np.random.default_rng(7)
    ps = [rng.standard_normal(h.keep_cols.size) for _ in range(2)]
    fs = _open(h, mask=mask)
    try:
        avail = fs.solver.cg_available(3)
        info = fs.solver.cg_scaled_info()
        layout = fs.solver.cg_layout_info()
        qs = [fs.solver.normal_apply(_full(fs, p))[fs.keep_cols] for p in ps]
        again = [fs.solver.normal_apply(_full(fs, p))[fs.keep_cols] for p in ps]
        A = fs.solver.get_csr()
    finally:
        fs.close()
    return h, mask, avail, info, layout, ps, qs, again, A


@pytest.mark.parametrize('name', NAMES)
def test_operator(gpu_available, name):
    h, mask, avail, info, layout, ps, qs, again, A = _operator(name)
    assert avail == (True, ''), avail
    assert layout['mode'] == 'column'
    assert info['parts'] == SH.SCALED_PARTS[name], info
    # one field entry per (y, x) centre of every scaled part
    want = sum(8 * W2.size for W2, uni in SH.part_fields(h, h.w) if not uni)
    assert info['field_bytes'] == want and info['grids'] == (2 if name == 'mask-maps' else 1), info
    _same_as_host(A, h.A(h.w, mask))
    for p, q, q2 in zip(ps, qs, again):
        ref = A.T @ (A @ p)
        err = float(np.max(np.abs(q - ref)) / np.max(np.abs(ref)))
        print(name, 'operator error', err)
        assert err <= OP_TOL
        assert np.array_equal(q, q2)   # fixed summation order, no atomics


@pytest.mark.parametrize('name', ['edges', 'maps-dz'])
def test_without_the_key_nothing_changes(gpu_available, name):
    h = SH.host(name)
    fs = _open(h, scaled=False)
    try:
        ok, why = fs.solver.cg_available(3)
        assert not ok and 'per-row scales' in why, why
        assert why == 'a stencil part has per-row scales (masked or non-uniform constraint rows)'
        assert fs.solver.cg_scaled_info() == dict(parts=0, field_bytes=0, grids=0, workgroups=0)
        x, st = fs.solver.solve(h.rhs, precond=3, method=1, **TIGHT)
        assert st['method'] == 0   # the LSQR fallback
        # the switch on the same handle: CGNR; off again: the refusal again
        fs.solver.set_cg_scaled(True)
        assert fs.solver.cg_available(3) == (True, '')
        fs.solver.set_cg_scaled(False)
        assert fs.solver.cg_available(3) == (False, why)
    finally:
        fs.close()
    _close(x, SH.exact(name)[2], f'{name} LSQR fallback')
    with pytest.raises(ValueError, match='set_cg_scaled'):
        fs2 = _open(h)
        try:
            fs2.solver.set_cg_scaled(1)
        finally:
            fs2.close()


def test_uniform_scales_are_untouched_by_the_key(gpu_available):
    """a system whose parts all share one scale: no scaled parts, the same x bit for bit with and without"""
    h = H.ksweep_host((9, 11), 300, 5)
    xs = []
    for scaled in (True, False):
        fs = _open(h, scaled=scaled)
        try:
            assert fs.solver.cg_available(3) == (True, '')
            assert fs.solver.cg_scaled_info()['parts'] == 0
            xs.append(fs.solver.solve(h.rhs, precond=3, method=1, **TIGHT)[0])
        finally:
            fs.close()
    np.testing.assert_array_equal(xs[0], xs[1])


# ---- 2. solve --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_solve(gpu_available, name):
    h = SH.host(name)
    fs = _open(h)
    try:
        x, st = fs.solver.solve(h.rhs, precond=3, method=1, **TIGHT)
        x2, st2 = fs.solver.solve(h.rhs, precond=3, method=1, **TIGHT)
        xj, stj = fs.solver.solve(h.rhs, precond=1, method=1, **TIGHT)
    finally:
        fs.close()
    assert st['method'] == 1 and st['istop'] in (1, 2), st
    print(name, 'iterations', st['iters'], 'jacobi', stj['iters'])
    _close(x, SH.exact(name)[2], name)
    assert np.array_equal(x, x2) and st['iters'] == st2['iters']   # a repeat is bit-identical
    assert stj['method'] == 1
    _close(xj, SH.exact(name)[2], name + ' jacobi')


# ---- 3. iterates -----------------------------------------------------------------------------------
def test_iterates(gpu_available):
    name = 'edges'
    h = SH.host(name)
    fs = _open(h)
    try:
        dev = _solves(fs.solver, h.rhs, H.KS)
        A = fs.solver.get_csr()
    finally:
        fs.close()
    _same_as_host(A, h.A())
    ref = Ref(A, h.w * h.rhs, H.block_factors(A, _blocks(h)), max(H.KS))
    _check_iterates('scaled-' + name, dev, ref)


# ---- 4. refresh ------------------------------------------------------------------------------------
def test_refresh_and_refusals(gpu_available):
    """the three masks at (21, 70, 5) share their lattice: another mask's constraint scales on the same handle"""
    h, h2 = SH.host('edges'), SH.host('checker')
    assert h.n_data != h2.n_data and h.w.size - h.n_data == h2.w.size - h2.n_data
    w2 = np.concatenate([h.w[:h.n_data], h2.w[h2.n_data:]])
    assert not np.array_equal(w2, h.w)
    rng = np.random.default_rng(23)
    p = rng.standard_normal(h.keep_cols.size)
    fs = _open(h)
    try:
        q1 = fs.solver.normal_apply(_full(fs, p))[fs.keep_cols]
        fs.solver.set_row_weight(w2)
        q2 = fs.solver.normal_apply(_full(fs, p))[fs.keep_cols]
        # weights that differ along t at one node of one part: refused, naming the part; method 1 → LSQR
        rows = h.S['Gc'].TOC['rows']['grad2_dzdt']
        w3 = h.w.copy()
        w3[h.n_data + rows[len(rows) // 2]] *= 1.5
        fs.solver.set_row_weight(w3)
        ok, why = fs.solver.cg_available(3)
        x3, st3 = fs.solver.solve(h.rhs, precond=3, method=1, **TIGHT)
        # precond 4 with legitimate scales: its own reason
        fs.solver.set_row_weight(h.w)
        ok3 = fs.solver.cg_available(3)
        ok4, why4 = fs.solver.cg_available(4)
        with pytest.raises(NativeError, match='multigrid: per-row constraint scales'):
            fs.solver.solve(h.rhs, precond=4, method=1, **TIGHT)
        q1b = fs.solver.normal_apply(_full(fs, p))[fs.keep_cols]
    finally:
        fs.close()
    for q, w in ((q1, h.w), (q2, w2)):
        A = h.A(w)
        ref = A.T @ (A @ p)
        err = float(np.max(np.abs(q - ref)) / np.max(np.abs(ref)))
        print('refresh: operator error', err)
        assert err <= OP_TOL
    assert np.array_equal(q1, q1b) and not np.array_equal(q1, q2)
    assert not ok and 'differ along dim 2' in why and 'stencil part' in why, why
    part = [k for k, (_, _, row0, lo, hi, _, _) in enumerate(SH.stencil_parts(h))
            if row0 <= rows[len(rows) // 2] < row0 + int(np.prod(np.subtract(hi, lo)))]
    assert f'stencil part {part[0]} ' in why, (part, why)
    assert st3['method'] == 0
    A3 = h.A(w3)
    _close(x3, ls_solve_dense(A3, w3 * h.rhs), 'scales that differ along t: LSQR')
    assert ok3 == (True, '')
    assert not ok4 and why4 == 'multigrid: per-row constraint scales', why4


# ---- 5. smooth_fit ---------------------------------------------------------------------------------
def _disc():
    yy, xx = np.meshgrid(np.arange(64), np.arange(64), indexing='ij')
    return (yy - 32) ** 2 + (xx - 32) ** 2 > 15 ** 2


def _fit(**kw):
    D, base = synthetic.points('t64')
    args = dict(base, mask_data=_disc(), max_iterations=1, VERBOSE=False, lsq_dense_max=0)
    args.update(kw)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        return LS.smooth_fit(data=D, **args)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _plain_fits():
    return _fit(lsq_cg_scaled=True), _fit()


def test_smooth_fit_disc_mask(gpu_available):
    on, off = _plain_fits()
    assert on['timing']['cg_scaled'] is True and on['timing']['lsq_last']['method'] == 1
    assert on['timing']['lsq_last']['precond'] == 3      # 'auto' takes block-Jacobi
    assert off['timing']['cg_scaled'] is False and off['timing']['lsq_last']['method'] == 0
    for f, a, b in (('z0', on['m']['z0'].z0, off['m']['z0'].z0), ('dz', on['m']['dz'].dz, off['m']['dz'].dz)):
        r = _rel(a, b)
        print(f'disc mask, {f}: with against without the key {r:.2e}')
        assert r <= 1e-6
    with pytest.raises(NativeError, match='multigrid: per-row constraint scales'):
        _fit(lsq_cg_scaled=True, lsq_precond=4)


def _exact_m(S, reference_epoch):
    """z0 / dz of the exact LS solution of the fit objects' system (every data row kept; columns behind
    the grids', the biases, are kept too)"""
    from lssurf_amd.constraint_functions import reference_epoch_keep_cols
    gz, gd = S['grids']['z0'], S['grids']['dz']
    G = sp.vstack([S['G_data'].toCSR(), S['Gc'].toCSR()]).tocsc()
    keep = reference_epoch_keep_cols(G.shape[1], gd, reference_epoch)
    w = 1. / np.concatenate((S['Ed'], S['Ec']))
    A = sp.csr_matrix(sp.diags(w) @ G[:, keep])
    m = np.zeros(G.shape[1])
    m[keep] = ls_solve_dense(A, w * S['rhs'])
    return m[gz.col_0:gz.col_0 + gz.N_nodes].reshape(gz.shape), m[gd.col_0:gd.col_0 + gd.N_nodes].reshape(gd.shape)


def _against_oracle(S, objs, reference_epoch, tag):
    z0, dz = _exact_m(objs, reference_epoch)
    for f, a, b in (('z0', S['m']['z0'].z0, z0), ('dz', S['m']['dz'].dz, dz)):
        r = _rel(a, b)
        print(f'{tag}, {f}: against the dense oracle {r:.2e}')
        assert r <= 1e-6


def _with_sensors(D):
    D.assign(sensor=(np.arange(D.size) % 3).astype(float), sigma_corr=np.full(D.size, 0.5))
    return D


def test_smooth_fit_eliminated_biases(gpu_available):
    """bias_params with lsq_bias='eliminate' on the masked fit: raises without the key, runs with it.  On
    t64 (49 152 columns: no dense factor in a few seconds) against the fit that carries the biases as columns
    and solves by LSQR; against the dense oracle on the 'edges' system of scaled_host (7 353 columns)."""
    D, base = synthetic.points('t64')
    D = _with_sensors(D)
    args = dict(base, mask_data=_disc(), max_iterations=1, VERBOSE=False, lsq_dense_max=0, bias_params=['sensor'])
    with pytest.raises(NativeError) as e:
        LS.smooth_fit(data=D, lsq_bias='eliminate', **args)
    print('without the key:', e.value)
    assert 'per-row scales' in str(e.value)
    S = LS.smooth_fit(data=D, lsq_bias='eliminate', lsq_cg_scaled=True, **args)
    assert S['timing']['cg_scaled'] is True and S['timing']['lsq_last']['method'] == 1
    C = LS.smooth_fit(data=D, lsq_bias='columns', **args)
    assert C['timing']['cg_scaled'] is False and C['timing']['lsq_last']['method'] == 0
    for f, a, b in (('z0', S['m']['z0'].z0, C['m']['z0'].z0), ('dz', S['m']['dz'].dz, C['m']['dz'].dz)):
        r = _rel(a, b)
        print(f't64 eliminated biases, {f}: against the columns fit {r:.2e}')
        assert r <= 1e-6
    D2, kw2 = SH.points('edges')
    D2 = _with_sensors(D2)
    args2 = dict(kw2, max_iterations=1, VERBOSE=False, lsq_dense_max=0, bias_params=['sensor'])
    S2 = LS.smooth_fit(data=D2, lsq_bias='eliminate', lsq_cg_scaled=True, **args2)
    assert S2['timing']['cg_scaled'] is True and S2['timing']['lsq_last']['method'] == 1
    objs = LS.smooth_fit(data=D2, return_fit_objects=True, lsq_bias='columns', **args2)
    _against_oracle(S2, objs, kw2['reference_epoch'], 'eliminated biases')


def test_smooth_fit_priors(gpu_available):
    """the dz prior of tests/golden/sys_prior_dz.npz (priors_common) on a masked fit: extra rows inside CGNR"""
    from conftest import golden, golden_points
    from priors_common import prior_kwargs
    g = golden('sys_prior_dz.npz')
    kw = dict(prior_kwargs(g), max_iterations=1, VERBOSE=False, lsq_dense_max=0)
    objs0 = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, **kw)
    ny, nx = (int(v) for v in objs0['grids']['dz'].shape[:2])
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing='ij')
    kw['mask_data'] = (yy - ny // 2) ** 2 + (xx - nx // 2) ** 2 > 4 ** 2
    objs = LS.smooth_fit(data=golden_points(g), return_fit_objects=True, **kw)
    assert np.unique(objs['Ec'][objs['Gc'].TOC['rows']['grad2_dzdt']]).size == 2
    with warnings.catch_warnings():
        warnings.simplefilter('error')   # no triplet path
        S = LS.smooth_fit(data=golden_points(g), lsq_cg_scaled=True, **kw)
    assert S['timing']['cg_scaled'] is True and S['timing']['lsq_last']['method'] == 1
    _against_oracle(S, objs, kw['reference_epoch'], 'dz prior')


def test_smooth_fit_three_iterations(gpu_available):
    S = _fit(lsq_cg_scaled=True, max_iterations=3)
    assert S['timing']['cg_scaled'] is True and len(S['timing']['lsq_iters_per_solve']) >= 2
    assert np.all(np.isfinite(S['m']['dz'].dz))
