"""Block-Jacobi CGNR (lsq method 1, precond 3; lsqr_cg.inc, block.hip) iterate for iterate against
tests/cgnr_host.py: textbook PCG with the node-block factors rounded to bf16 as the device rounds
them, in extended precision.  A solve with zero tolerances stops at maxit = k alone, so x_k of
k ∈ {1, 2, 3, 4, 5, 7, 8, 9, 13} shows the iterate with 1, 2, 3 and no owed α p of the deferred x
update (CG_XK = 4, k_cg_xfix), in the first x cycle and in later ones.

Tolerance: e_k = ‖x_k^f64 − x_k^ld‖ / ‖x_k‖ is the reference's own float64-against-extended spread;
the device must stay within τ_k = max(1000·e_k, 1e-13) of the extended-precision iterate.  The
factor 1000 covers the device's other association of the stencil sums and its sums over workgroup
partials (the suite grants the operator alone 1e-12); a defect of the block normals, the factor,
the bf16 rounding or the deferred x moves the iterates by 1e-5 and more (the sensitivity tests).
The host R_b⁻¹ and the device's agree only to rounding: tests/test_cgnr_host.py asserts that no
entry of any input used here lies where that could change its bf16 value.

Every case runs its device solves BEFORE get_csr(): forming the full CSR switches the block normals
to k_block_normal.  The figures go to the file named by CGNR_ITERATES_JSON, when set
(profiles/cgnr_iterates.json is one such run)."""
import atexit
import contextlib
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import conftest  # noqa: F401  (puts the repository root on sys.path, also in the child process)
import cgnr_host as H

pytestmark = pytest.mark.gpu
KS, KS9 = H.KS, H.KS9
ZERO = dict(atol=0.0, btol=0.0, method=1)
EST = ('r1norm', 'arnorm', 'xnorm', 'anorm')
EST_TOL = 1e-10

RECORD = {}


def _dump_record():
    path = os.environ.get('CGNR_ITERATES_JSON')
    if path and RECORD:
        with open(path, 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


atexit.register(_dump_record)


@contextlib.contextmanager
def _env(name, value):
    saved = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if saved is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = saved


def _solves(solver, rhs, ks, precond=3, x0=None, **kw):
    """{k: (x_k, stats)}: only maxit stops a solve with zero tolerances"""
    out = {}
    for k in ks:
        x, st = solver.solve(rhs, x0=x0, maxit=k, precond=precond, **ZERO, **kw)
        assert st['method'] == 1 and st['istop'] == 7 and st['iters'] == k, st
        out[k] = (x, st)
    return out


class Ref:
    """The reference iterates of one system in float64 and extended precision, e_k and τ_k."""

    def __init__(self, A, b, factors, kmax, x0=None):
        self.A, self.b, self.factors, self.x0 = A, b, factors, x0
        self.f64 = H.pcg(A, b, factors, kmax, x0=x0)
        self.ld = H.pcg(A, b, factors, kmax, x0=x0, dtype=np.longdouble)
        assert self.ld['x'].dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18
        self.e = {k: self.dev(k, self.f64['x'][k]) for k in range(1, kmax + 1)}
        self.tau = {k: max(1000 * e, 1e-13) for k, e in self.e.items()}

    def dev(self, k, x, ref=None):
        """‖x − x_k^ld‖ / ‖x_k^ld‖"""
        return H.rel(np.asarray(x).astype(np.longdouble), self.ld['x'][k] if ref is None else ref)

    def stats(self, k):
        return H.stats_at(self.A, self.b, self.factors, self.f64['x'][k], self.x0, self.f64['alpha'][:k],
                          self.f64['beta'][:k])


def _open(h, w=None, mask=None, **kw):
    fs = h.fit_system(**kw)
    try:
        assert fs.formation == 'stencil' and fs.has_blocks
        fs.solver.set_row_weight(h.w if w is None else w)
        fs.solver.set_row_mask(np.ones(fs.n_data + fs.n_con, bool) if mask is None else mask)
        ok, why = fs.solver.cg_available(3)
        assert ok, why
    except BaseException:
        fs.close()
        raise
    return fs


def _same_as_host(A, A_host):
    """get_csr() is the host-formed A whose factor entries test_cgnr_host.py found clear of every bf16
    rounding boundary (within 1e-11 relative)"""
    assert A.shape == A_host.shape and abs(A - A_host).max() <= 1e-12 * abs(A).max()


def _blocks(h):
    return H.block_list(*h.blocks, h.keep_cols.size)


@functools.lru_cache(maxsize=None)
def _t64():
    """t64 with every row kept: the device iterates of the three block-normal kernels (class tables,
    part descriptors with LSQ_BLK_TAB=0, the full CSR's k_block_normal) and of precond 1, and the
    references from the formed A.  Shared, never changed."""
    h = H.synthetic_host('t64')
    dev = {}
    fs = _open(h)
    try:
        dev['t64'] = _solves(fs.solver, h.rhs, KS)
        dev['jacobi'] = _solves(fs.solver, h.rhs, KS9, precond=1)
        A = fs.solver.get_csr()
        fs.solver.set_row_weight(h.w)          # the factors again, now from the formed GT
        dev['t64-csr'] = _solves(fs.solver, h.rhs, KS9)
    finally:
        fs.close()
    with _env('LSQ_BLK_TAB', '0'):             # read at every block_normal call
        fs = _open(h)
        try:
            dev['t64-mf'] = _solves(fs.solver, h.rhs, KS9)
        finally:
            fs.close()
    _same_as_host(A, h.A())
    b = h.w * h.rhs
    ref = Ref(A, b, H.block_factors(A, _blocks(h)), 20)
    refj = Ref(A, b, H.jacobi_factors(A), 9)
    return h, dev, ref, refj


@functools.lru_cache(maxsize=None)
def _t64_mask():
    h = H.synthetic_host('t64')
    w, mask = H.mask_and_weights(h)
    fs = _open(h, w, mask)
    try:
        dev = _solves(fs.solver, h.rhs, KS9)
        A = fs.solver.get_csr()
    finally:
        fs.close()
    _same_as_host(A, h.A(w, mask))
    return h, dev, Ref(A, (w * h.rhs)[mask], H.block_factors(A, _blocks(h)), 9), (w, mask)


@functools.lru_cache(maxsize=None)
def _t64_x0():
    h, _, ref, _ = _t64()
    x0 = H.warm_start(h)
    fs = _open(h)
    try:
        dev = _solves(fs.solver, h.rhs, KS9, x0=x0)
    finally:
        fs.close()
    return h, dev, Ref(ref.A, ref.b, ref.factors, 9, x0=x0)


def _plain(h):
    """device solves of a system with its own weights and every row kept, then the reference"""
    fs = _open(h)
    try:
        dev = _solves(fs.solver, h.rhs, KS9)
        A = fs.solver.get_csr()
    finally:
        fs.close()
    _same_as_host(A, h.A())
    return dev, Ref(A, h.w * h.rhs, H.block_factors(A, _blocks(h)), 9)


@functools.lru_cache(maxsize=None)
def _priors():
    """t64 plus the frame rows of test_gpu_priors._frame_priors(1e-4) as the device's extra rows; the
    reference's A is the host vstack of a plain handle's get_csr() and the weighted X."""
    from test_gpu_priors import _frame_priors
    h, _, ref, _ = _t64()
    csr, wx, prior = _frame_priors(1e-4)
    mine = H.frame_priors(h, h.S['grids']['dz'].shape[2] // 2)
    assert all(np.array_equal(a, b) for a, b in zip(csr, mine[0]))
    assert np.array_equal(wx, mine[1]) and np.array_equal(prior, mine[2])
    W, b = np.r_[h.w, wx], np.r_[h.rhs, prior]
    fs = _open(h, W, np.ones(W.size, bool), extra_csr=csr)
    try:
        assert fs.n_extra == wx.size
        dev = _solves(fs.solver, b, KS9)
    finally:
        fs.close()
    A = sp.vstack([ref.A, H.extra_rows_host(h, csr, wx)]).tocsr()
    return h, dev, Ref(A, W * b, H.block_factors(A, _blocks(h)), 9)


def _case(name):
    """(device {k: (x, stats)}, Ref) of a case of the table"""
    if name in ('t64', 't64-mf', 't64-csr', 'jacobi'):
        _, dev, ref, refj = _t64()
        return dev[name], refj if name == 'jacobi' else ref
    if name == 't64-mask':
        return _t64_mask()[1:3]
    if name == 't64-x0':
        return _t64_x0()[1:3]
    if name == 'priors':
        return _priors()[1:3]
    if name == 'sf3d':
        return _plain(H.golden_host('sf3d'))
    return _plain(H.synthetic_host(name))


def _check_iterates(name, dev, ref):
    rec = RECORD.setdefault(name, {})
    bad = []
    for k, (x, _) in sorted(dev.items()):
        d = ref.dev(k, x)
        rec[str(k)] = dict(device=d, e_k=ref.e[k], tau_k=ref.tau[k])
        print(f'{name} k={k}: device {d:.2e}, e_k {ref.e[k]:.2e}, tau_k {ref.tau[k]:.2e}')
        if not d <= ref.tau[k]:
            bad.append((k, d, ref.tau[k]))
    assert not bad, (name, bad)


# path reached (block.hip, lsqr_cg.inc), per case:
#   t64      k_block_normal_tab, k_block_factor_k<12>, k_cg_block<true,12,5> (4 096 % 5 = 1: a last wave
#            step with one block)
#   t64-mf   k_block_normal_mf (LSQ_BLK_TAB=0)          t64-csr  k_block_normal (after get_csr)
#   t64-mask block normals and operator under a row mask and re-weighted data rows
#   t64-x0   r0 = b − A x0                               sf3d     6-column blocks, edge tiles only
#   t15      k_block_factor, k_cg_block<true,BJ_LANES>  t64z     k_cg_block<false,BJ_LANES>, 11 + 1 columns
#   priors   k_xr_blk_mark, k_xr_blk_add                jacobi   k_cg_jacobi with the deferred x
@pytest.mark.parametrize('name', ['t64', 't64-mf', 't64-csr', 't64-mask', 't64-x0', 'sf3d', 't15', 't64z', 'priors',
                                  'jacobi'])
def test_iterates_match_host_reference(gpu_available, name):
    dev, ref = _case(name)
    assert sorted(dev) == list(KS if name == 't64' else KS9)
    _check_iterates(name, dev, ref)


@pytest.mark.parametrize('nt', H.KSWEEP_NT)
def test_iterates_block_size_sweep(gpu_available, nt):
    """Node blocks of k = nt columns, 2 … 13: every k another number of blocks per wave (64 / k), on a
    lattice inside one 64-node strip (9 × 11) and on one that crosses into a second (7 × 70)."""
    for shape, npts in H.KSWEEP:
        h = H.ksweep_host(shape, npts, nt)
        assert h.keep_cols.size == shape[0] * shape[1] * nt and np.all(np.diff(h.blocks[0]) == nt)
        dev, ref = _plain(h)
        _check_iterates(f'ksweep-{shape[0]}x{shape[1]}-{nt}', dev, ref)


@pytest.mark.parametrize('name', ['t64', 't64-mask', 't64-x0'])
def test_estimates_match_their_definitions(gpu_available, name):
    """r1norm (rn2 −= αρ), arnorm, the preconditioned xnorm (dn2, dp, pn2) and anorm (trace of the
    Lanczos T) of k_cg_alpha / k_cg_beta against stats_at at every k, 1e-10 relative: the recurrence
    of r1norm loses ε·k·(‖r0‖/‖r_k‖)² ≈ 4e-13 on t64, the other three are sums of positive terms."""
    dev, ref = _case(name)
    bad = []
    for k, (_, st) in sorted(dev.items()):
        want = ref.stats(k)
        for f in EST:
            err = abs(st[f] - want[f]) / want[f]
            print(f'{name} k={k} {f}: device {st[f]!r}, host {want[f]!r}, rel {err:.2e}')
            if not err <= EST_TOL:
                bad.append((k, f, st[f], want[f]))
        plain = float(np.linalg.norm(ref.f64['x'][k]))
        assert abs(plain - want['xnorm']) > 0.1 * want['xnorm']      # ‖x‖ would not pass for xnorm
    assert not bad, bad


def test_graph_replay_stops_where_eager_steps_stop(gpu_available):
    """use_graph True / False at k = 2, 5, 8: the steps of a replayed batch behind the stop are
    no-ops, so both give the same x bit for bit."""
    h, dev, _, _ = _t64()
    fs = _open(h)
    try:
        eager = _solves(fs.solver, h.rhs, (2, 5, 8), use_graph=False)
    finally:
        fs.close()
    for k in (2, 5, 8):
        np.testing.assert_array_equal(eager[k][0], dev['t64'][k][0])
        for f in EST:
            assert eager[k][1][f] == dev['t64'][k][1][f], (k, f)


def test_batch_size_does_not_change_the_iterate(gpu_available):
    h, dev, _, _ = _t64()
    fs = _open(h)
    try:
        for batch in (4, 8, 16):
            x, st = fs.solver.solve(h.rhs, maxit=7, precond=3, batch=batch, **ZERO)
            assert st['istop'] == 7 and st['iters'] == 7
            np.testing.assert_array_equal(x, dev['t64'][7][0])
    finally:
        fs.close()


def test_iterate_calls_continue_one_run(gpu_available):
    """lsq_iterate: 5 then 4 steps stand at the reference's step 9; 20 steps with batch = 16 (one
    replayed batch and four eager steps) at its step 20."""
    h, _, ref, _ = _t64()
    got = {}
    fs = _open(h)
    try:
        fs.solver.iterate(h.rhs, 5, precond=3, method=1)
        got[9] = fs.solver.iterate(h.rhs, 4, precond=3, method=1)
    finally:
        fs.close()
    fs = _open(h)
    try:
        got[20] = fs.solver.iterate(h.rhs, 20, precond=3, method=1, batch=16)
    finally:
        fs.close()
    for k, st in got.items():
        want = ref.stats(k)
        assert st['iters'] == k and st['method'] == 1
        for f in ('r1norm', 'arnorm'):
            err = abs(st[f] - want[f]) / want[f]
            print(f'iterate to {k} {f}: rel {err:.2e}')
            assert err <= EST_TOL, (k, f, st[f], want[f])


def test_separate_row_and_column_reads_of_the_factor(gpu_available, tmp_path):
    """k_cg_block<true,12,13>, the default above 2 M node blocks, forced at t64's size by
    LSQ_CG_BLOCK_RC=0 (a function-local static: one fresh child process; LSQ_CG_NT unset).  Nothing
    in the ABI says which instantiation ran, so this proves only that the forced setting computes
    the reference's iterates."""
    h, _, ref, _ = _t64()
    env = dict(os.environ, LSQ_CG_BLOCK_RC='0')
    env.pop('LSQ_CG_NT', None)
    out = tmp_path / 'x.npz'
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--rc-child', str(out)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    _check_iterates('t64-rc0', {k: (got[f'x{k}'], None) for k in KS}, ref)


def _child(path):
    assert os.environ.get('LSQ_CG_BLOCK_RC') == '0' and 'LSQ_CG_NT' not in os.environ
    h = H.synthetic_host('t64')
    fs = _open(h)
    try:
        dev = _solves(fs.solver, h.rhs, KS)
    finally:
        fs.close()
    np.savez(path, **{f'x{k}': x for k, (x, _) in dev.items()})


# ---- sensitivity: the device against a deliberately altered REFERENCE -------------------------
def test_sensitivity_unrounded_factors(gpu_available):
    """Exact factors in the reference: the device is more than 1e3·τ_k away at every k."""
    h, dev, ref, _ = _t64()
    xe = H.pcg(ref.A, ref.b, H.block_factors(ref.A, _blocks(h), round=False), 13, dtype=np.longdouble)['x']
    for k in KS:
        d = ref.dev(k, dev['t64'][k][0], xe[k])
        assert d > 1e3 * ref.tau[k], (k, d, ref.tau[k])


def test_sensitivity_dropped_owed_step(gpu_available):
    """A reference whose x lacks the second step's α p (a deferred term never paid)."""
    _, dev, ref, _ = _t64()
    for k in (2, 3):
        xb = ref.ld['x'][k] - ref.ld['alpha'][1] * ref.ld['p'][1]
        d = ref.dev(k, dev['t64'][k][0], xb)
        assert d > 1e3 * ref.tau[k], (k, d, ref.tau[k])


def test_sensitivity_block_normals_that_ignore_the_mask(gpu_available):
    """A reference whose factors come from every row although the operator is masked, from the
    first k at which the two references differ by more than 1e3·τ_k (x_1 is α_0 M⁻¹s_0)."""
    h, dev, ref, (w, mask) = _t64_mask()
    Aall = sp.csr_matrix(sp.diags(w) @ h.G)
    xb = H.pcg(ref.A, ref.b, H.block_factors(Aall, _blocks(h)), 9, dtype=np.longdouble)['x']
    apart = {k: ref.dev(k, xb[k]) for k in KS9}
    print('masked against unmasked factors:', {k: f'{v:.2e}' for k, v in apart.items()})
    first = min(k for k in KS9 if apart[k] > 1e3 * ref.tau[k])
    assert first <= 2
    for k in KS9:
        if k >= first:
            d = ref.dev(k, dev[k][0], xb[k])
            assert d > 1e3 * ref.tau[k], (k, d, ref.tau[k])


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--rc-child':
        _child(sys.argv[2])
