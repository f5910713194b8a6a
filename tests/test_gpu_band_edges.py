"""The band factor's edges against host references (tests/band_host.py; the inputs' own conditions
are pinned in tests/test_band_host.py).

precond 5's triangular solves (k_band_bsub, k_band_fsub, k_band_warm) were tested only through
converged LSQR solves, which a roughly right preconditioner passes too.  With an exact factor A·M has
orthonormal columns, so ONE LSQR step from any start returns the least-squares solution: x after
maxit=1 is compared with the refined host x* at max(32·e_host, 64·(w+1)·ε·κ), e_host the float64
host's error of the same step.  The cases reach the strided loops of both kernels (w > NW), every
LSQ_BAND_NW regime (child processes: the switch is read once), n a multiple of 64, w clipped to
T − 1, and a ring of more than 64 KiB of dynamic LDS.

The batched window factorization (band_cov_windows_batched, the default LSQ_E_FBATCH = 8 without op
rows) is compared with the host's conditional σ on bands of different T and w in one launch, a last
batch of one window, and Schur splits beside plain windows.

With BAND_EDGES_JSON set the figures go to that file (profiles/band_edges.json is one such run of
this file alone)."""
import atexit
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import conftest  # noqa: F401
import band_host as H
from lssurf_amd._native import ptr
from lssurf_amd.solver import LSQSolver

pytestmark = pytest.mark.gpu
RECORD = {}


def _dump_record():
    path = os.environ.get('BAND_EDGES_JSON')
    if path and RECORD:
        with open(path, 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


atexit.register(_dump_record)


def _name(n, reach, tag=''):
    return f'{n}-{reach}' + (f'-{tag}' if tag else '')


def _nw(w, cap=H.NW_DEFAULT):
    return max(1, min(w, cap))


def _rec(name, F, quantity, e_host, dev, bnd, cap=H.NW_DEFAULT):
    r = RECORD.setdefault(name, {'n': F.n, 'T': F.T, 'w': F.w, 'NW': _nw(F.w, cap), 'kappa': F.kappa})
    r[quantity] = {'e_host': e_host, 'device': dev, 'bound': bnd}   # e_host None: a fixed project bound
    print(f'{name} {quantity}: e_host {e_host if e_host is None else format(e_host, ".2e")} device {dev:.2e} '
          f'bound {bnd:.2e}')


def _open(A, perm=None):
    s = LSQSolver(0)
    try:
        C = sp.coo_matrix(A)
        s.set_matrix_coo(C.shape[0], C.shape[1], C.row, C.col, C.data)
        if perm is not None:
            s.set_band_order(perm)
    except BaseException:
        s.close()
        raise
    return s


def _perm(F, order):
    return F.perm.astype(np.int32) if order == 'block' else None


def _one_step(name, F, A, b, tag, x1, st1, x2, st2, cap=H.NW_DEFAULT):
    """check 2 on a device's (x, stats) of maxit=1 and of the converged solve"""
    xs = F.xstar(b)
    e_host = H.rel_err(H.host_one_step(A, b, F), xs)
    bnd = H.bound(e_host, F.w, F.kappa)
    dev = H.rel_err(x1, xs)
    _rec(name, F, f'x1-{tag}', e_host, dev, bnd, cap)
    _rec(name, F, f'x-converged-{tag}', e_host, H.rel_err(x2, xs), bnd, cap)
    assert st1['iters'] == 1, st1
    assert dev <= bnd, (name, tag, dev, bnd)
    assert st2['istop'] in (1, 2) and st2['iters'] <= 2, st2


def _check2(s, name, F, A):
    for tag, b in zip(('random', 'edge'), H.edge_rhs(A, F.perm)):
        x1, st1 = s.solve(b, precond=5, maxit=1)
        x2, st2 = s.solve(b, precond=5, atol=1e-12, btol=1e-12)
        _one_step(name, F, A, b, tag, x1, st1, x2, st2)


# ---- 1. factor shape sweep ------------------------------------------------------------------------
SWEEP = [(n, r, 'natural') for n, r in H.SMALL] + [(768, 190, 'block'), (897, 514, 'block')]


@pytest.mark.parametrize('n,reach,order', SWEEP)
def test_factor_shapes(gpu_available, n, reach, order):
    A, F, _, _ = H.case(n, reach, order)
    perm = _perm(F, order)
    with _open(A) as s:
        info = np.zeros(3, np.int64)
        s._check(s._L.lsq_band_factor(s._h, ptr(perm) if perm is not None else None, ptr(info), None, None, None),
                 'lsq_band_factor')
        R, po = s.band_factor(perm)
    assert tuple(info) == (n, F.T, F.w)
    if order == 'natural':
        assert (F.T, F.w) == H.CASES[(n, reach)]
    assert np.array_equal(po, F.perm)
    R = R.tocoo()
    assert np.all(R.row <= R.col) and np.all(R.tocsr().diagonal() > 0)
    assert np.all((R.col >> 6) - (R.row >> 6) <= F.w)          # nothing outside the band
    D = (R.T @ R).toarray() - F.N
    assert np.abs(D).max() / np.abs(F.N).max() <= 1e-12


# ---- 2. one step is exact -------------------------------------------------------------------------
@pytest.mark.parametrize('n,reach,order', SWEEP)
def test_one_step_is_exact(gpu_available, n, reach, order):
    A, F, _, _ = H.case(n, reach, order)
    with _open(A, _perm(F, order)) as s:
        _check2(s, _name(n, reach, '' if order == 'natural' else order), F, A)


@pytest.mark.parametrize('n,reach', [(897, 514), (65, 3)])
def test_one_step_after_reweight_and_mask(gpu_available, n, reach):
    """set_row_weight / set_row_mask behind a solve: the band is refactored for the new rows."""
    A, F0, _, _ = H.case(n, reach)
    _, F, w_rows, keep = H.case(n, reach, reweight=True)
    b = H.edge_rhs(A)[0]
    with _open(A) as s:
        x, st = s.solve(b, precond=5, maxit=1)                   # the factor for unit weights
        assert H.rel_err(x, F0.xstar(b)) < 1e-11
        s.set_row_weight(w_rows)
        s.set_row_mask(keep)
        _check2(s, _name(n, reach, 'reweighted'), F, A)


# ---- 3. warm start --------------------------------------------------------------------------------
@pytest.mark.parametrize('n,reach', [(65, 3), (897, 514), (1536, 1028)])
def test_warm_start(gpu_available, n, reach):
    A, F, _, _ = H.case(n, reach)
    b = H.edge_rhs(A)[0]
    xs = F.xstar(b)
    xs64 = xs.astype(np.float64)
    x0 = np.random.default_rng([n, 17]).standard_normal(n) * np.linalg.norm(xs64) / np.sqrt(n)
    with _open(A) as s:
        xa, sta = s.solve(b, x0=xs64, precond=5)
        xb, stb = s.solve(b, x0=x0, precond=5, maxit=1)
    for tag, start, x in (('warm-xstar', xs64, xa), ('warm-random', x0, xb)):
        e_host = H.rel_err(H.host_one_step(A, b, F, x0=start), xs)
        bnd = H.bound(e_host, F.w, F.kappa)
        dev = H.rel_err(x, xs)
        _rec(_name(n, reach), F, tag, e_host, dev, bnd)
        assert dev <= bnd, (tag, dev, bnd)
    assert stb['iters'] == 1, stb


# ---- 4. LSQ_BAND_NW -------------------------------------------------------------------------------
_CHILD_NW = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import scipy.sparse as sp
import band_host as H
from lssurf_amd.solver import LSQSolver
A = H.banded_system(int(sys.argv[4]), int(sys.argv[5]))
out = {}
with LSQSolver(0) as s:
    C = sp.coo_matrix(A)
    s.set_matrix_coo(C.shape[0], C.shape[1], C.row, C.col, C.data)
    for tag, b in zip(('random', 'edge'), H.edge_rhs(A)):
        x1, st1 = s.solve(b, precond=5, maxit=1)
        x2, st2 = s.solve(b, precond=5, atol=1e-12, btol=1e-12)
        out['x1_' + tag], out['x2_' + tag] = x1, x2
        out['st_' + tag] = np.array([st1['iters'], st1['istop'], st2['iters'], st2['istop']])
np.savez(sys.argv[3], **out)
'''


def test_band_nw_values(gpu_available, tmp_path):
    """LSQ_BAND_NW = 1 (no barrier, every tile in the strided loop), 3 (17 = 5·3 + 2: uneven) and 64
    (clipped to w: no stride) on (1536, 1028): one child process per value, each x against the host
    x*, never against another child's."""
    n, reach = 1536, 1028
    A, F, _, _ = H.case(n, reach)
    here = os.path.dirname(os.path.abspath(__file__))
    for nw in ('1', '3', '64'):
        path = tmp_path / f'nw{nw}.npz'
        r = subprocess.run([sys.executable, '-c', _CHILD_NW, here, os.path.dirname(here), str(path), str(n), str(reach)],
                           env=dict(os.environ, LSQ_BAND_NW=nw), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        z = np.load(path)
        for tag, b in zip(('random', 'edge'), H.edge_rhs(A)):
            st = [int(v) for v in z['st_' + tag]]
            _one_step(_name(n, reach, 'NW' + nw), F, A, b, tag, z['x1_' + tag], {'iters': st[0], 'istop': st[1]},
                      z['x2_' + tag], {'iters': st[2], 'istop': st[3]}, cap=int(nw))


# ---- 5. the wide case -----------------------------------------------------------------------------
def test_wide_ring_above_64k(gpu_available):
    """(8391, 8260): w = 130, a ring of 131·512 = 67 072 B of dynamic LDS in both solve kernels.
    No factor download; x* from the host's LAPACK factor of the same normal matrix plus the
    longdouble refinement step (band_host.xstar_lu, the sparse LU, agrees with it to 4 ε on the
    smaller cases and takes a minute at this size: the band is full)."""
    n, reach = H.WIDE
    A, F, _, _ = H.case(n, reach)
    assert (F.T, F.w) == H.CASES[H.WIDE] and (F.w + 1) * 64 * 8 > 64 * 1024
    with _open(A) as s:
        _check2(s, _name(n, reach), F, A)


# ---- 6. E at the edges ----------------------------------------------------------------------------
def _edge_ops(n, T, w, seed):
    """130 op rows (three sweep workgroups, the last partly filled): single columns (the ends and
    the tile edges among them), local rows, rows spanning more than w tiles (the whole range)."""
    rng = np.random.default_rng([seed, n])
    rows = []
    single = [0, n - 1] + [c for c in (63, 64, 127, 128, n - 2) if 0 <= c < n]
    single += list(rng.integers(0, n, 40 - len(single)))
    rows += [([c], [1.0]) for c in single]
    for _ in range(45):
        c0 = int(rng.integers(0, max(1, n - 4)))
        c = np.arange(c0, min(n, c0 + 4))
        rows.append((c, rng.uniform(0.1, 1.0, c.size)))
    for _ in range(45):
        mid = np.unique(rng.integers(0, n, 3))
        c = np.unique(np.r_[rng.integers(0, min(64, n)), mid, n - 1 - rng.integers(0, min(64, n))])
        rows.append((c, rng.uniform(0.1, 1.0, c.size)))
    ri = np.concatenate([np.full(len(c), i) for i, (c, _) in enumerate(rows)])
    op = sp.csr_matrix((np.concatenate([v for _, v in rows]), (ri, np.concatenate([c for c, _ in rows]))),
                       shape=(len(rows), n))
    assert op.shape[0] == 130
    return op


@pytest.mark.parametrize('n,reach', [(64, 20), (65, 3), (129, 128), (897, 514), (1536, 1028)])
def test_E_at_the_edges(gpu_available, n, reach):
    A, F, _, _ = H.case(n, reach)
    op = _edge_ops(n, F.T, F.w, 5)
    with _open(A) as s:
        E, oe, info = s.cov_band(None, op)
    assert (int(info[1]), int(info[0])) == (F.T, F.w)
    ref = H.window_sigma(F.N, np.arange(n))
    ref_inv = np.sqrt(np.diag(np.linalg.inv(F.N)))
    ref_op = H.op_sigma(F.N, op)
    dE, dO = float(np.max(np.abs(E / ref - 1))), float(np.max(np.abs(oe / ref_op - 1)))
    _rec(_name(n, reach), F, 'E', float(np.max(np.abs(ref_inv / ref - 1))), dE, 1e-11)
    _rec(_name(n, reach), F, 'E-op-rows', None, dO, 1e-11)
    assert dE <= 1e-11 and dO <= 1e-11, (dE, dO)


# ---- 7. mixed batches -----------------------------------------------------------------------------
def _mixed_windows(n):
    """Nine contiguous column ranges of 40 … n columns at assorted offsets (tile-aligned and not),
    inner None, a middle third (whole tiles left unswept), or a single column."""
    sizes = [40, 64, 65, 128, 200, 449, 700, min(1000, n), n]
    offs = [3, 64, 127, 0, 301, 64, 5, 0, 0]
    wins = []
    for k, (sz, a) in enumerate(zip(sizes, offs)):
        a = min(a, n - sz)
        cols = np.arange(a, a + sz, dtype=np.int32)
        if k in (0, 3, 8):
            inner = None
        elif k == 5:
            inner = np.arange(sz) == 300
        else:
            inner = (np.arange(sz) >= sz // 3) & (np.arange(sz) < 2 * sz // 3)
        wins.append((cols, inner, None))
    return wins


@pytest.mark.parametrize('n,reach', [(1536, 1028), (768, 190)])
def test_mixed_window_batches(gpu_available, n, reach):
    """cov_band_windows without op rows takes the batched factorization: nine windows are two
    batches, the second of one window; T and w differ inside a launch (the guards K < b.T,
    blockIdx.x < min(b.w, b.T − 1 − K) and c > m of the k_band_*_b kernels)."""
    assert 'LSQ_E_FBATCH' not in os.environ
    A, F, _, _ = H.case(n, reach)
    wins = _mixed_windows(n)
    shapes = {H.tile_width(A, cols) for cols, _, _ in wins}
    assert len({T for T, _ in shapes}) >= 5 and len({w for _, w in shapes}) >= 3
    with _open(A) as s:
        Eb, _, info = s.cov_band_windows(wins)
        alone = [s.cov_band_window(cols, inner=inner)[0] for cols, inner, _ in wins]
    worst = 0.0
    for (cols, inner, _), e, ea in zip(wins, Eb, alone):
        ref = H.window_sigma(F.N, cols, inner)
        on = np.ones(cols.size, bool) if inner is None else inner
        assert np.all(e[~on] == 0.0)
        worst = max(worst, float(np.max(np.abs(e[on] / ref[on] - 1))))
        np.testing.assert_array_equal(e, ea)
    _rec(_name(n, reach), F, 'windows-batched', None, worst, 1e-11)
    assert worst <= 1e-11, worst
    assert int(info[1]) == F.T and int(info[0]) == F.w          # the widest band of the batches


# ---- 8. Schur windows in a mixed batch ------------------------------------------------------------
def test_schur_windows_in_a_mixed_batch(gpu_available):
    n, reach = 768, 190
    assert 'LSQ_E_FBATCH' not in os.environ
    A, F, _, _ = H.case(n, reach)
    C = sp.csr_matrix(A)
    # (a, c, mb, nib): the window [a, c), its bottom margin Mb = [c − mb, c), Ib the nib columns before
    split = [(0, 400, 60, 190), (100, 768, 128, 200), (37, 500, 65, 190), (200, 650, 1, 190), (0, 768, 200, 256)]
    plain = [(5, 69), (300, 600), (639, 768)]
    wins, whole = [], []
    for k, (a, c, mb, nib) in enumerate(split):
        assert nib >= reach and c - mb - nib >= a
        # no live row holds a column of A \ Ib and one of Mb
        in_top = (C.indices >= a) & (C.indices < c - mb - nib)
        in_mb = (C.indices >= c - mb) & (C.indices < c)
        assert not np.any(np.logical_or.reduceat(in_top, C.indptr[:-1]) & np.logical_or.reduceat(in_mb, C.indptr[:-1]))
        perm_A = np.arange(a, c - mb, dtype=np.int32)
        perm_B = np.arange(c - mb - nib, c, dtype=np.int32)[::-1].copy()
        na = perm_A.size
        inner = None if k == 0 else (np.arange(na) >= na // 3) & (np.arange(na) < na - 7 * k)
        wins.append((perm_A, inner, perm_B, nib))
        whole.append(np.arange(a, c))
    for a, c in plain:
        wins.append((np.arange(a, c, dtype=np.int32), None, None, 0))
        whole.append(np.arange(a, c))
    order = [0, 5, 1, 2, 6, 3, 7, 4]                               # split and plain windows interleaved
    with _open(A) as s:
        Es, info = s.cov_band_windows_schur([wins[i] for i in order])
    worst = 0.0
    for i, e in zip(order, Es):
        perm_A, inner, _, _ = wins[i]
        ref = H.window_sigma(F.N, whole[i])[:perm_A.size]
        on = np.ones(perm_A.size, bool) if inner is None else inner
        assert e.size == perm_A.size and np.all(e[~on] == 0.0)
        worst = max(worst, float(np.max(np.abs(e[on] / ref[on] - 1))))
    _rec(_name(n, reach), F, 'windows-schur', None, worst, 1e-9)
    assert worst <= 1e-9, worst
