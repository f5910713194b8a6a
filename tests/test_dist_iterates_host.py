"""tests/dist_host.py (TEST INFRASTRUCTURE of tests/test_gpu_dist_iterates.py) kept honest on the CPU,
and the justification of that test's bar.

* Every (system, ranks) pair of the GPU test plans on the host without error: the ranks' rows tile the
  system's rows once, every rank owns at least one node row, and the slab heights are the ones the
  tables name (one-row slabs on the 7 × 70 lattice with 4 and 7 ranks and on 5 × 200 with 5); the
  ranks' halo lists mirror each other.
* The rule that splits coarse multigrid levels over ranks, restated on the host, gives the levels the
  GPU test expects to be partitioned, and its row ranges tile every level.
* No block-factor entry of a system new to the iterate tests (ksweep-5x200-13, ta64) lies where host
  and device could round to different bf16 values.
* Each slab defect a rank-boundary bug would amount to moves some x_k, k ≤ 3, of the host reference by
  at least 100·τ_k (measured: 1e9 to 3e12·τ_k) on 33x33-5 with 2 ranks and 7x70-8 with 3: block normals
  of one slab's nodes without the other ranks' rows, column norms from the owner's rows only, the
  level-0 restriction or prolongation without its entries across a cut, λ from one slab's rows, and
  for LSQR a ghost ṽ left at its previous value."""
import functools

import numpy as np
import pytest

import cgnr_host as H
import dist_host as D
import lsqr_host as LH
import mg_host as M
from test_gpu_cgnr_iterates import Ref

F64, LD = np.float64, np.longdouble
PAIRS = D.all_pairs()
DEFECT_ON = [('33x33-5', 2), ('7x70-8', 3)]


@pytest.mark.parametrize('name,nranks,rows', PAIRS, ids=[f'{n}-{r}' for n, r, _ in PAIRS])
def test_every_pair_plans_and_tiles_the_rows(name, nranks, rows):
    h = D.inputs(name)[0]
    plans = D.plan(name, nranks)
    assert D.owned_rows(name, nranks) == rows and min(rows) >= 1
    assert sum(rows) == int(h.S['grids']['dz'].shape[0])
    got = np.sort(np.concatenate([p['rows'] for p, _ in plans]))
    assert np.array_equal(got, np.arange(h.w.size))                       # every row on one rank, once
    own = np.zeros(h.keep_cols.size, int)
    for p, _ in plans:
        x = np.zeros(h.keep_cols.size)
        from lssurf_amd.dist import window_owned_solution
        window_owned_solution(p, np.ones(p['keep'].size), x)
        own += x.astype(int)
        assert p['halo'] == 1 and p['m'] == p['rows'].size
    assert np.all(own == 1)                                               # every column owned once
    # what r sends to p is what p receives from r: the same global columns in the same order
    for r, (p, (peers, scnt, sidx, rcnt, ridx)) in enumerate(plans):
        so = np.r_[0, np.cumsum(scnt)]
        for i, q in enumerate(peers):
            pq, (peers_q, _, _, rcnt_q, ridx_q) = plans[q]
            j = int(np.flatnonzero(peers_q == r)[0])
            ro = np.r_[0, np.cumsum(rcnt_q)]
            assert np.array_equal(p['l2g'][sidx[so[i]:so[i + 1]]], pq['l2g'][ridx_q[ro[j]:ro[j + 1]]])


def test_t64z_has_no_global_description():
    """two lattices (z0 refined): multigrid over ranks is refused there, CGNR and LSQR are not"""
    assert all(p['glob'] is None for p, _ in D.plan('t64z', 2))
    assert all(p['glob'] is not None for p, _ in D.plan('t64', 2))
    assert all(len(p['fields']) == 1 for p, _ in D.plan('ta64', 3))


def _levels(name):
    h = D.inputs(name)[0]
    ny, nx, nt = (int(v) for v in h.S['grids']['dz'].shape)
    rows = [ny]
    while max(ny, nx) > 5 and not (len(rows) > 1 and ny * nx * (1 + nt) <= 1024):      # mg_host.hierarchy's rule
        ny, nx = ny // 2 + 1, nx // 2 + 1
        rows.append(ny)
    return rows


# (system, ranks, LSQ_MG_PART_MIN, LSQ_MG_PART) -> lp.  33x33-5 has three levels (33, 17 and the coarsest, 9
# rows: 486 columns ≤ MG_COARSE_COLS), and the coarsest is never split: one partitioned level at most.
WANT_LP = {('t64', 2, 8, True): 2, ('t64', 3, 8, True): 1, ('t64', 4, 8, True): 1, ('t64', 8, 8, True): 0,
           ('33x33-5', 2, 8, True): 1, ('7x70-8', 2, 8, True): 0, ('7x70-8', 3, 8, True): 0, ('23x38-3', 3, 8, True): 0,
           ('33x33-5', 3, 2, True): 1, ('33x33-5', 4, 2, True): 1, ('t64', 3, 2, True): 3, ('t64', 2, 8, False): 0}


@pytest.mark.parametrize('key', list(WANT_LP), ids=[f'{k[0]}-{k[1]}-min{k[2]}-{"on" if k[3] else "off"}' for k in WANT_LP])
def test_partitioned_levels_on_the_host(key):
    name, nranks, pmin, on = key
    rows = _levels(name)
    assert rows == [lv[0][0] for lv in M.case_system(name).lev[F64]] if name != 't64' else rows == [64, 33, 17, 9, 5]
    bounds = [0] + [int(v) for v in np.cumsum(D.owned_rows(name, nranks))]
    lp, own = D.mg_partition(rows[0], bounds, rows, pmin, on)
    assert lp == WANT_LP[key], (lp, own)
    for l, ranges in enumerate(own):                        # every level tiled without gap or overlap
        assert ranges[0][0] == 0 and ranges[-1][1] == rows[l]
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))


@pytest.mark.parametrize('name', ['ksweep-5x200-13', 'ta64'])
def test_new_hosts_have_no_factor_entry_near_a_rounding_boundary(name):
    """the condition of tests/test_cgnr_host.py on the systems this suite adds to the iterate tests"""
    h = D.inputs(name)[0]
    A, _ = D.system(name)
    ent = H.factor_entries(H.block_factors(A, D.blocks(h), round=False))     # also asserts the pivots
    assert H.at_risk_entries(ent) == 0


# ---- the slab defects ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cg_ref(name, precond):
    h = D.inputs(name)[0]
    A, b = D.system(name)
    return Ref(A, b, H.block_factors(A, D.blocks(h)) if precond == 3 else H.jacobi_factors(A), 3)


def _assert_moved(what, moved):
    print(what, {k: f'{v:.1e}' for k, v in moved.items()})
    assert max(moved.values()) >= 100, (what, moved)


@pytest.mark.parametrize('name,nranks', DEFECT_ON)
def test_sensitivity_block_normals_of_one_slab_alone(name, nranks):
    A, b = D.system(name)
    ref = _cg_ref(name, 3)
    for rank in range(nranks):
        xs = H.pcg(A, b, D.bj_local(name, nranks, rank), 3, dtype=LD)['x']
        _assert_moved(f'{name} bj_local rank {rank}', {k: ref.dev(k, xs[k]) / ref.tau[k] for k in (1, 2, 3)})


@pytest.mark.parametrize('name,nranks', DEFECT_ON)
def test_sensitivity_column_norms_from_the_owner_alone(name, nranks):
    A, b = D.system(name)
    ref = _cg_ref(name, 1)
    xs = H.pcg(A, b, D.jac_local(name, nranks), 3, dtype=LD)['x']
    _assert_moved(f'{name} jac_local', {k: ref.dev(k, xs[k]) / ref.tau[k] for k in (1, 2, 3)})


@functools.lru_cache(maxsize=None)
def _mg_ref(name):
    A, b = D.system(name)
    S = M.case_system(name)
    lam = [float(v) for v in S.host_lambda()]
    x64 = M.pcg_v(A, b, S.compact(S.cycle(lam, F64)), 3)
    xld = M.pcg_v(A, b, S.compact(S.cycle(lam, LD)), 3, dtype=LD)
    return S, lam, xld, {k: max(1000 * H.rel(x64[k].astype(LD), xld[k]), 1e-13) for k in (1, 2, 3)}


@pytest.mark.parametrize('which', ['restrict_cut', 'prolong_cut', 'lam_local'])
@pytest.mark.parametrize('name,nranks', DEFECT_ON)
def test_sensitivity_multigrid_across_a_cut(name, nranks, which):
    A, b = D.system(name)
    S, lam, xld, tau = _mg_ref(name)
    V, lam2 = D.mg_defect_cycle(S, lam, LD, which, name, nranks)
    if which == 'lam_local':
        assert abs(lam2[0] / lam[0] - 1) > 1e-3 and lam2[1:] == lam[1:]
    xs = M.pcg_v(A, b, S.compact(V), 3, dtype=LD)
    _assert_moved(f'{name} {which}', {k: H.rel(xs[k], xld[k]) / tau[k] for k in (1, 2, 3)})


@pytest.mark.parametrize('precond', [0, 1])
@pytest.mark.parametrize('name,nranks', DEFECT_ON)
def test_sensitivity_stale_ghost_v(name, nranks, precond):
    """stale_v of tests/lsqr_host.py on the ghost columns alone; active from k = 2 (w_1 = v_1)"""
    A, b = D.system(name)
    f = LH.identity_factors(A.shape[1]) if precond == 0 else H.jacobi_factors(A)
    ref = LH.Ref(A, b, f, 3)
    ghost = D.ghost_columns(name, nranks)
    assert 0 < ghost.sum() < ghost.size          # the node rows beside a cut, not every column
    xs = LH.lsqr(A, b, f, 3, dtype=LD, defect='stale_v', stale_cols=ghost)['x']
    _assert_moved(f'{name} stale ghost v', {k: ref.dev(k, xs[k]) / ref.tau[k] for k in (2, 3)})
