"""LSQR (lsq method 0; lsqr.hip, lsqr_mf.inc, lsqr_block.inc) iterate for iterate against
tests/lsqr_host.py: Paige & Saunders' LSQR on A·M from the definitions in extended precision, M = 1
(precond 0), 1/‖A_j‖ (precond 1) or the node-block factors rounded to bf16 as the device rounds them
(precond 3).  A solve with zero tolerances stops at maxit = k alone, so x_k and the five recurrence
scalars of k ∈ K = (1, 2, 3, 15, 16, 17, 32, 33) show, with the default batch of 16, a stop on the
first, a middle and the last iteration of a batch (the last one's owed x/w update is paid by
launch_flush, the others' by the next launch of the batch), both parities of the ṽ buffers, the first
batch and the third.  Both operators: op 0, the structured kernels in the full column space with
zv = cs∘ṽ, and op 1, the SELL kernels whose stored values carry cs.

Tolerance: e_k = ‖x_k^f64 − x_k^ld‖ / ‖x_k^ld‖ is the reference's own float64-against-extended spread;
the device must stay within τ_k = max(1000·e_k, 1e-13) of the extended-precision iterate, and every
scalar (r1norm, anorm, acond, arnorm, xnorm) within the same construction with floor 1e-12.  The
factor 1000 is the one tests/test_gpu_cgnr_iterates.py grants for the device's other association of
the stencil sums and its sums over workgroup partials; the defects these tests are there for (a
factor entry one bf16 step off, M for Mᵀ, a row weight, a dropped template entry, an owed update
never paid, a stale ṽ, cs applied twice) move x_k by more than 100·τ_k (tests/test_lsqr_host.py,
which also asserts that no factor entry of any case lies where host and device could round apart).
Largest device/τ_k seen (profiles/lsqr_iterates.json, 31 case × operator × preconditioner entries):
0.0063 for x_k (sf3d as triplets, precond 0) and 0.0024 for a scalar (arnorm, t64-x0 op 0 precond 1,
k = 17): the device stays within a few e_k of the extended-precision iterate.  e_k is 2e-16 to 7e-15
everywhere but on ksweep-7x70-13, whose Lanczos vectors lose orthogonality from k ≈ 20 (e_33 = 3.4e-13,
the device 1.1e-13 from the reference there).

Which side of MF_LDS_MAX (4096 doubles of staged zv bands per block; lsqr_host.lds_sums): every z0
grid takes 1542 and every dz grid but one 1545 to 1578, so their A·v is staged in LDS; the dz grid
of `hbm` (5 × 9 nodes, 860 epochs) would take 4119 and gathers from HBM, beside its staged z0 grid.

Every case runs its op 0 solves first and never asks for get_csr() before them: forming the full CSR
switches the block normals to k_block_normal.  The host A is cgnr_host.Host.A.  The figures go to
the file named by LSQR_ITERATES_JSON, when set (profiles/lsqr_iterates.json is one such run)."""
import atexit
import functools
import json
import os

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the repository root on sys.path)
import lsqr_host as L

pytestmark = pytest.mark.gpu
K, K4, KB = L.K, L.K4, L.KB
KW = (1, 2, 3, 16, 17)             # warm start and hbm: a stop mid-batch, on the flush, in the second batch
ZERO = dict(atol=0.0, btol=0.0, conlim=0.0, method=0)

RECORD = {}


def _dump_record():
    path = os.environ.get('LSQR_ITERATES_JSON')
    if path and RECORD:
        with open(path, 'w') as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


atexit.register(_dump_record)


def _solves(solver, rhs, ks, precond, op, x0=None, **kw):
    """{k: (x_k, stats)}: only maxit stops a solve with zero tolerances"""
    out = {}
    for k in ks:
        x, st = solver.solve(rhs, x0=x0, maxit=k, precond=precond, op=op, **ZERO, **kw)
        assert st['method'] == 0 and st['istop'] == 7 and st['iters'] == k, st
        out[k] = (x, st)
    return out


def _open(c, grids=True):
    """The structured system of case c with its weights and mask."""
    from lssurf_amd.smooth_fit import FitSystem
    h = c.h
    fs = FitSystem(h.S['G_data'], h.S['Gc'], h.keep_cols, h.n_full, grids=h.S['grids'] if grids else None)
    try:
        assert fs.formation == 'stencil' and fs.solver.info()['stencil_op'] == 1
        fs.solver.set_row_weight(c.w)
        fs.solver.set_row_mask(c.mask)
    except BaseException:
        fs.close()
        raise
    return fs


# case: ((op, precond) combinations in the order run — op 0 first —, the k of every combination)
PLAN = {
    't64': ([(op, p) for op in (0, 1) for p in (0, 1, 3)], K),
    't64-mask': ([(op, p) for op in (0, 1) for p in (1, 3)], K4),
    't64-rows': ([(op, p) for op in (0, 1) for p in (1, 3)], K4),
    't64-x0': ([(op, p) for op in (0, 1) for p in (1, 3)], KW),
    'ta64': ([(0, 1), (0, 3)], K4),
    'hbm': ([(0, 0), (0, 1)], KW),
}
PLAN.update({name: ([(0, 3)], K) for name in L.SMALL})


@functools.lru_cache(maxsize=None)
def _dev(name):
    """{(op, precond): {k: (x, stats)}} of a structured case; afterwards get_csr() must be the host's A."""
    c = L.case(name)
    combos, ks = PLAN[name]
    fs = _open(c, grids=name != 'hbm')
    try:
        out = {(op, p): _solves(fs.solver, c.h.rhs, ks, p, op, x0=c.x0) for op, p in combos}
        A = fs.solver.get_csr()
    finally:
        fs.close()
    assert A.shape == c.A.shape and abs(A - c.A).max() <= 1e-12 * abs(A).max()
    return out


@functools.lru_cache(maxsize=None)
def _dev_coo():
    """sf3d's host-formed A handed over as triplets (no structure: S.mf is false, every op runs the
    SELL kernels), its node blocks through set_column_blocks."""
    import lssurf_amd as LS
    c = L.case('sf3d')
    coo = c.A.tocoo()
    with LS.LSQSolver(0) as s:
        s.set_matrix_coo(c.A.shape[0], c.A.shape[1], coo.row, coo.col, coo.data)
        assert s.info()['stencil_op'] == 0
        s.set_column_blocks_csr(*c.h.blocks)
        return {(0, p): _solves(s, c.b, K, p, 0) for p in (0, 1, 3)}


def _check(tag, dev, ref):
    """x_k within τ_k and the five scalars within theirs, at every k; the figures into RECORD."""
    rec = RECORD.setdefault(tag, {})
    bad = []
    for k, (x, st) in sorted(dev.items()):
        d = ref.dev(k, x)
        row = dict(device=d, e_k=ref.e[k], tau_k=ref.tau[k], ratio=d / ref.tau[k])
        print(f'{tag} k={k}: device {d:.2e}, e_k {ref.e[k]:.2e}, tau_k {ref.tau[k]:.2e}')
        if not d <= ref.tau[k]:
            bad.append((k, 'x', d, ref.tau[k]))
        for f in L.SCALARS:
            ds = ref.sdev(f, k, st[f])
            row[f] = dict(device=ds, e_k=ref.es[f][k], tau_k=ref.taus[f][k])
            print(f'{tag} k={k} {f}: device {ds:.2e}, e_k {ref.es[f][k]:.2e}, tau_k {ref.taus[f][k]:.2e}')
            if not ds <= ref.taus[f][k]:
                bad.append((k, f, ds, ref.taus[f][k]))
        rec[str(k)] = row
    rec['largest_ratio'] = max(r['ratio'] for r in rec.values() if isinstance(r, dict))
    assert not bad, (tag, bad)


def _params(names):
    return [pytest.param(n, op, p, id=f'{n}-op{op}-p{p}') for n in names for op, p in PLAN[n][0]]


# path reached, per case:
#   t64       op 0: k_mf_fwd (staged bands, constant part scales), k_mf_spmtv, k_mf_init_u, k_mf_x; op 1: k_xw_spmv,
#             k_spmtv, k_init_u, k_scale; precond 3: k_block_epi (bf16 lf_t copy), k_block_x
#   t64-mask  the operators under a row mask and re-weighted data rows (parts keep one row scale)
#   t64-rows  per-row rs in mf_fwd_part and mf_at_part (wconst = 0 for every part)
#   t64-x0    k_mf_warm, k_block_warm, k_scale with divide, u0 = b − A x0
#   ta64      the field-valued part (VAR, NT = MF_MAXT: 9 entries)
#   hbm       k_mf_fwd's HBM gather (LDS = false) for dz beside the staged z0
@pytest.mark.parametrize('name,op,precond', _params(['t64', 't64-mask', 't64-rows', 't64-x0', 'ta64', 'hbm']))
def test_iterates_match_host_reference(gpu_available, name, op, precond):
    dev = _dev(name)[(op, precond)]
    assert sorted(dev) == list(PLAN[name][1])
    _check(f'{name}/op{op}/p{precond}', dev, L.case(name).ref(precond, max(dev)))


@pytest.mark.parametrize('name', L.SMALL)
def test_iterates_small_and_odd_grids(gpu_available, name):
    """op 0, precond 3 on grids below one MF_ALIGN block of 512 nodes (9 × 11 × 2: 198 dz nodes), with
    row counts that are no multiple of 64 or 512 (lin2d alone has 46 full slices of 64 rows: 2944),
    node blocks of 2, 5, 6, 8 and 13 columns, and 2-D grids padded to three dimensions (lin2d: z0
    alone, singleton blocks; nb_xt: a 3 × 101 lattice)."""
    c = L.case(name)
    dev = _dev(name)[(0, 3)]
    assert sorted(dev) == list(K)
    assert c.h.n_data % 64 and c.h.n_full % 512 and c.A.shape[0] % 512
    assert (c.A.shape[0] % 64 == 0) == (name == 'lin2d')
    _check(f'{name}/op0/p3', dev, c.ref(3, max(K)))


@pytest.mark.parametrize('precond', [0, 1, 3])
def test_iterates_generic_formation(gpu_available, precond):
    dev = _dev_coo()[(0, precond)]
    _check(f'sf3d-coo/p{precond}', dev, L.case('sf3d').ref(precond, max(K)))


def test_cases_fall_on_both_sides_of_the_lds_limit(gpu_available):
    """The rule of assemble.hip restated on the host (lsqr_host.lds_sums): hbm's dz grid alone exceeds
    MF_LDS_MAX, every other grid of every case is staged."""
    over = {}
    for name in PLAN:
        for grid, total in L.case(name).lds().items():
            print(f'{name} {grid}: {total}')
            if total > L.MF_LDS_MAX:
                over[(name, grid)] = total
    assert over == {('hbm', 'dz'): 3 * (L.MF_ALIGN + L.HBM_NT + 1)}


# ---- batching, lsq_iterate, b_rows: bit for bit ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def _t64_open():
    """One t64 handle shared by the bit-for-bit tests (closed at exit)."""
    fs = _open(L.case('t64'))
    atexit.register(fs.close)
    return fs


@pytest.mark.parametrize('op', [0, 1])
def test_batching_changes_nothing(gpu_available, op):
    """x_k of k = 1 … 5 bit for bit across batch 2, 3 (rounded to 4) and 16, replayed graph or eager
    launches: stops mid-batch and on the last iteration of a batch (batch 2: k = 2, 4; batch 4: k = 4)."""
    fs, rhs = _t64_open(), L.case('t64').h.rhs
    base = _dev('t64')[(op, 3)]
    ref = None
    for batch in (2, 3, 16):
        for use_graph in (True, False):
            got = _solves(fs.solver, rhs, KB, 3, op, batch=batch, use_graph=use_graph)
            ref = got if ref is None else ref
            for k in KB:
                np.testing.assert_array_equal(got[k][0], ref[k][0], err_msg=f'batch {batch} graph {use_graph} k {k}')
                for f in L.SCALARS:
                    assert got[k][1][f] == ref[k][1][f], (batch, use_graph, k, f)
    for k in (1, 2, 3):                    # and the solves of test_iterates_match_host_reference
        np.testing.assert_array_equal(ref[k][0], base[k][0])


def _fresh(fs, rhs):
    """a solve consumes the iteration state: the next iterate() starts anew"""
    fs.solver.solve(rhs, maxit=1, **ZERO)


def _same_scalars(a, b, what):
    for f in L.SCALARS + ('iters',):
        assert a[f] == b[f], (what, f, a[f], b[f])


@pytest.mark.parametrize('op,precond', [(0, 1), (0, 3), (1, 1), (1, 3)])
def test_iterate_scalars_are_the_solves(gpu_available, op, precond):
    """lsq_iterate(k) from a fresh state stands where lsq_solve(maxit = k) stopped, bit for bit."""
    fs, rhs = _t64_open(), L.case('t64').h.rhs
    base = _dev('t64')[(op, precond)]
    for k in K:
        _fresh(fs, rhs)
        _same_scalars(fs.solver.iterate(rhs, k, precond=precond, op=op), base[k][1], k)


@pytest.mark.parametrize('op,precond', [(0, 3), (1, 3), (0, 1)])
def test_iterate_carries_an_odd_parity_into_a_full_batch(gpu_available, op, precond):
    """3 + 16 + 1 steps (the 16 run eagerly from parity 1) against 20 in one call (a replayed batch
    of 16 and 4 eager steps)."""
    fs, rhs = _t64_open(), L.case('t64').h.rhs
    _fresh(fs, rhs)
    whole = fs.solver.iterate(rhs, 20, precond=precond, op=op)
    _fresh(fs, rhs)
    assert fs.solver.iterate(rhs, 3, precond=precond, op=op)['iters'] == 3
    assert fs.solver.iterate(rhs, 16, precond=precond, op=op)['iters'] == 19
    _same_scalars(fs.solver.iterate(rhs, 1, precond=precond, op=op), whole, '3 + 16 + 1')
    assert whole['iters'] == 20


def test_iterate_starts_anew_when_preconditioner_or_operator_changes(gpu_available):
    fs, rhs = _t64_open(), L.case('t64').h.rhs
    _fresh(fs, rhs)
    want = {(op, p): None for op in (0, 1) for p in (1, 3)}
    for key in want:
        _fresh(fs, rhs)
        want[key] = fs.solver.iterate(rhs, 5, precond=key[1], op=key[0])
    _fresh(fs, rhs)
    for a, b in [((0, 3), (0, 1)), ((0, 1), (1, 1)), ((1, 1), (1, 3)), ((1, 3), (0, 3))]:
        fs.solver.iterate(rhs, 5, precond=a[1], op=a[0])
        _same_scalars(fs.solver.iterate(rhs, 5, precond=b[1], op=b[0]), want[b], (a, b))


@pytest.mark.parametrize('op', [0, 1])
def test_b_rows_equals_the_full_rhs(gpu_available, op):
    """b_rows = n_data: the constraint rows' zeros stay on the host; same x bit for bit."""
    c = L.case('t64')
    fs = _t64_open()
    assert not c.h.rhs[c.h.n_data:].any()
    base = _dev('t64')[(op, 3)]
    for k in (3, 16, 17):
        x, st = fs.solver.solve(c.h.rhs, maxit=k, precond=3, op=op, b_rows=c.h.n_data, **ZERO)
        np.testing.assert_array_equal(x, base[k][0])
        _same_scalars(st, base[k][1], k)
