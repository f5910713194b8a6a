"""Host side of the y-slab ranks' iterate tests (tests/test_gpu_dist_iterates.py, tests/
test_dist_iterates_host.py): the table of (system, rank count) cases with the slab heights each must
give, their inputs (weights, row mask, warm start) from the Hosts of tests/cgnr_host.py, mg_host.py and
lsqr_host.py, the plan of every rank (lssurf_amd.dist.window_problem / window_halo, no device), a host
restatement of the rule that splits coarse multigrid levels over ranks (group_mg_partition in
lsqr_cg_dist.inc), and the slab defects the iterate tests are there to catch, emulated on the host
references.  Test infrastructure only."""
import functools

import numpy as np
import scipy.sparse as sp

import cgnr_host as H
import lsqr_host as LH
import mg_host as M

# ---- the cases ---------------------------------------------------------------------------------
# CGNR with block-Jacobi (precond 3) and Jacobi (precond 1): system -> {ranks: owned dz node rows per rank}
CG_CASES = {
    'ksweep-7x70-8': {2: (4, 3), 3: (2, 3, 2), 4: (2, 2, 1, 2), 7: (1,) * 7},   # two x tiles; down to one row per rank
    'ksweep-9x11-5': {2: (4, 5), 4: (2, 2, 3, 2)},                              # a lattice narrower than one tile
    'ksweep-5x200-13': {2: (2, 3), 5: (1,) * 5},             # x tiles clear of both edges, 16-long register columns
    't64': {2: (32, 32), 3: (21, 22, 21), 8: (8,) * 8},      # odd cuts (21, 43) with 3 ranks
    't64-mask': {3: (21, 22, 21)},                           # row mask, data weights, warm start
    't15': {3: (27, 26, 27)},                                # 15 epochs: the ring kernel on windows
    't64z': {2: (32, 32), 3: (21, 22, 21)},                  # z0 on a refined lattice: two lattices, one y bound
    'ta64': {3: (21, 22, 21)},                               # field-valued parts sliced per rank
}
# CGNR with multigrid (precond 4): system -> {ranks: owned rows}; MG_LP: the partitioned levels expected
MG_CASES = {
    't64': {2: (32, 32), 3: (21, 22, 21), 4: (16,) * 4, 8: (8,) * 8},
    't64-mask': {3: (21, 22, 21)},
    '33x33-5': {2: (16, 17)},
    '7x70-8': {2: (4, 3), 3: (2, 3, 2)},
    '23x38-3': {3: (8, 7, 8)},
}
# children of the multigrid tests: (system, ranks, environment) and the owned rows
MG_CHILDREN = {
    '33x33-5/3/min2': ('33x33-5', 3, {'LSQ_MG_PART_MIN': '2'}),
    '33x33-5/4/min2': ('33x33-5', 4, {'LSQ_MG_PART_MIN': '2'}),
    't64/3/min2': ('t64', 3, {'LSQ_MG_PART_MIN': '2'}),
    't64/2/part0': ('t64', 2, {'LSQ_MG_PART': '0'}),
}
MG_CHILD_ROWS = {'33x33-5/3/min2': (11, 11, 11), '33x33-5/4/min2': (8, 8, 9, 8), 't64/3/min2': (21, 22, 21),
                 't64/2/part0': (32, 32)}
# LSQR over ranks (method 0, precond 0 and 1), structured and assembled ranks
LSQR_CASES = {'t64': {2: (32, 32), 3: (21, 22, 21)}, 't64-mask': {3: (21, 22, 21)}, 'ksweep-9x11-5': {4: (2, 2, 3, 2)}}
MG_KS = (1, 2, 3, 5, 8)
MG_PART_MIN = 8            # lsqr_cg_dist.inc


def all_pairs():
    """every (system, ranks, owned rows) of the tables above, once"""
    seen = {}
    for table in (CG_CASES, MG_CASES, LSQR_CASES):
        for name, by in table.items():
            for nr, rows in by.items():
                assert seen.setdefault((name, nr), rows) == rows
    for tag, (name, nr, _) in MG_CHILDREN.items():
        assert seen.setdefault((name, nr), MG_CHILD_ROWS[tag]) == MG_CHILD_ROWS[tag]
    return sorted((n, r, rows) for (n, r), rows in seen.items())


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(Host, row weights, row mask over every row, warm start or None) of a system name: `-mask`
    applies cgnr_host.mask_and_weights, and t64-mask also starts from cgnr_host.warm_start."""
    base = name[:-5] if name.endswith('-mask') else name
    if base == 'ta64':
        h = LH.case('ta64').h
    elif base in M.LATTICES:
        h = M.case_host(base)[0]
    elif base.startswith('ksweep'):
        h = H.host_case(base)[0]
    else:
        h = H.synthetic_host(base)
    if name.endswith('-mask'):
        w, mask = H.mask_and_weights(h)
        return h, w, mask, H.warm_start(h)
    return h, h.w, np.ones(h.w.size, bool), None


def system(name):
    """(A, b): the weighted, row-selected operator and right-hand side of inputs(name), host-formed"""
    h, w, mask, _ = inputs(name)
    return h.A(w, mask), (w * h.rhs)[mask]


def blocks(h):
    return H.block_list(*h.blocks, h.keep_cols.size)


# ---- the ranks' plan, on the host -----------------------------------------------------------------
def partition(h, nranks):
    from lssurf_amd import dist
    dz = [g for g in (p['grid'] for p in h.S['Gc'].parts) if g.N_dims == 3]
    return dist.SlabPartition(dz[0] if dz else h.S['Gc'].parts[0]['grid'], nranks)


@functools.lru_cache(maxsize=None)
def plan(name, nranks):
    """[(window_problem, window_halo)] per rank of a system's partition"""
    from lssurf_amd import dist
    h = inputs(name)[0]
    part = partition(h, nranks)
    out = []
    for r in range(nranks):
        p = dist.window_problem(h.S['G_data'], h.S['Gc'], part, r, h.keep_cols)
        out.append((p, dist.window_halo(p['grid_objs'], part, r, p['halo'])))
    return out


def owned_rows(name, nranks):
    """per rank the number of dz node rows it owns"""
    return tuple(int(p['meta'][-1]['b'] - p['meta'][-1]['a']) for p, _ in plan(name, nranks))


def column_owner(name, nranks):
    """owner rank of every compact column"""
    from lssurf_amd import dist
    h = inputs(name)[0]
    return dist.column_owner(h.keep_cols, plan(name, nranks)[0][0]['grid_objs'], partition(h, nranks))


def ghost_columns(name, nranks):
    """compact columns some rank holds as a ghost copy"""
    h = inputs(name)[0]
    ghost = np.zeros(h.keep_cols.size, bool)
    for p, _ in plan(name, nranks):
        own = np.zeros(p['n_full'], bool)
        for a, b in p['own_ranges']:
            own[a:b] = True
        ghost[p['keep_global'][~own[p['keep']]]] = True
    return ghost


def mg_partition(ny, bounds, levels, pmin=MG_PART_MIN, on=True):
    """group_mg_partition restated: bounds = the ranks' fine row bounds [0, …, ny]; levels = the rows of
    every level (level 0 first, the coarsest last).  Returns (lp, [[(oa, ob) per rank] per level]) under
    the assumption that every level below the finest runs a row-range kernel and has a stencil reach of
    at most max(pmin, 2) rows, which holds for the systems here."""
    own = [[(bounds[r], bounds[r + 1]) for r in range(len(bounds) - 1)]]
    for l in range(1, len(levels)):
        prev, S0p, S0 = own[-1], levels[l - 1], levels[l]
        own.append([(0 if a == 0 else (a + 1) // 2, S0 if b == S0p else (b + 1) // 2) for a, b in prev])
    lp = 0
    for l in range(1, len(levels) - 1):
        if not on or len(bounds) < 3 or min(b - a for a, b in own[l]) < max(pmin, 2):
            break
        lp = l
    return lp, own


# ---- slab defects, on the host references ----------------------------------------------------------
def rank_rows(name, nranks, rank):
    """global row ids of the rows `rank` owns (every row kept: the defect tests run unmasked systems)"""
    return np.sort(plan(name, nranks)[rank][0]['rows'])


def bj_local(name, nranks, rank):
    """block factors whose blocks on `rank`'s nodes come from that rank's rows alone (a reverse halo
    of the block normals that never arrives), the other ranks' blocks from every row"""
    h = inputs(name)[0]
    A, _ = system(name)
    owner = column_owner(name, nranks)
    Ar = A[rank_rows(name, nranks, rank)]
    Nr = (Ar.T @ Ar).tocsr()
    out, changed = [], 0
    for C, Rg in H.block_factors(A, blocks(h)):
        mine = owner[C[:, 0]] == rank
        R = Rg.copy()
        if mine.any():
            R[mine] = H.normal_factors(Nr, [C[mine]])[0][1]
        changed += int(np.count_nonzero(np.any(R != Rg, axis=(1, 2))))
        out.append((C, R))
    assert changed > 0
    return out


def jac_local(name, nranks):
    """Jacobi factors with every column's norm from its owner's rows alone"""
    A, _ = system(name)
    owner = column_owner(name, nranks)
    n2 = np.zeros(A.shape[1])
    for r in range(nranks):
        Ar = A[rank_rows(name, nranks, r)]
        n2r = np.asarray(Ar.multiply(Ar).sum(axis=0)).ravel()
        n2[owner == r] = n2r[owner == r]
    assert n2.min() > 0
    return [(np.arange(A.shape[1])[:, None], (1.0 / np.sqrt(n2)).reshape(-1, 1, 1))]


def cut_prolongation(P, shape, nt, bounds, coarse_bounds):
    """P of level 0 without the entries that link a fine node row to a coarse node row another rank
    owns (a restriction whose reverse halo, or a prolongation whose forward halo, is missing)"""
    ny, nx = shape
    nyc = coarse_bounds[-1]
    nxc = nx // 2 + 1
    fine_row = np.concatenate([np.repeat(np.arange(ny), nx), np.repeat(np.arange(ny), nx * nt)])
    coarse_row = np.concatenate([np.repeat(np.arange(nyc), nxc), np.repeat(np.arange(nyc), nxc * nt)])
    fo = np.searchsorted(np.asarray(bounds[1:-1]), fine_row, side='right')
    co = np.searchsorted(np.asarray(coarse_bounds[1:-1]), coarse_row, side='right')
    Pc = P.tocoo()
    keep = fo[Pc.row] == co[Pc.col]
    assert 0 < np.count_nonzero(~keep) < keep.size
    return sp.csr_matrix((Pc.data[keep], (Pc.row[keep], Pc.col[keep])), shape=P.shape).astype(P.dtype)


def mg_defect_cycle(S, lam, dtype, which, name, nranks):
    """mg_host.VCycle of system S at λ with one slab defect: restrict_cut / prolong_cut (the level-0
    transfer without its entries across a cut), lam_local (level 0's λ from the power steps on rank 0's
    rows alone)."""
    h = inputs(name)[0]
    ny, nx, nt = (int(v) for v in h.S['grids']['dz'].shape)
    bounds = [0] + [int(v) for v in np.cumsum(owned_rows(name, nranks))]
    if which == 'lam_local':
        A, _ = system(name)
        lev0 = M.hierarchy(A[rank_rows(name, nranks, 0)], int(np.count_nonzero(rank_rows(name, nranks, 0) < h.n_data)),
                           h.keep_cols, ny, nx, nt)[0]
        lam = [float(M.power_lambda(lev0, S.factors[0], nt))] + list(lam[1:])
        return S.cycle(lam, dtype), lam
    V = S.cycle(lam, dtype)
    _, own = mg_partition(ny, bounds, [lv[0][0] for lv in S.lev[np.float64]])
    cb = [0] + [b for _, b in own[1]]
    Pcut = cut_prolongation(V.P[0], (ny, nx), nt, bounds, cb)
    V.P, V.Pup = list(V.P), list(V.Pup)
    if which == 'restrict_cut':
        V.P[0] = Pcut
    else:
        assert which == 'prolong_cut'
        V.Pup[0] = Pcut
    return V, lam
