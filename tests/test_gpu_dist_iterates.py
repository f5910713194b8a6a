"""The y-slab ranks' solvers (lsqr_dist.inc, lsqr_cg_dist.inc, lssurf_amd/dist.py) iterate for iterate
against the host references of the single-GPU iterate tests: cgnr_host.pcg (block-Jacobi and Jacobi
CGNR), mg_host.pcg_v with the host V-cycle (multigrid CGNR) and lsqr_host.lsqr (LSQR), in extended
precision.  All ranks run on one GPU as a VirtualDistFitSystem: the kernels, plans and exchange order
of the RCCL path, exchanges as device copies.  A solve with zero tolerances stops at maxit = k alone
(istop 7, iters k), so x_k is compared directly; one reference per system and preconditioner serves
every rank count, because the reference knows nothing of the partition.  A preconditioner that is
wrong only at slab boundaries stays symmetric positive definite and converges to the same solution
(what tests/test_gpu_dist.py checks); its iterates differ from the first step on.

Tolerance (the rule of tests/test_gpu_cgnr_iterates.py, unchanged): e_k = ‖x_k^f64 − x_k^ld‖ / ‖x_k^ld‖
of the reference, τ_k = max(1000·e_k, 1e-13); the ranks add one more association of the sums
(per-rank partials, then rank order).  The CGNR estimates within 1e-10 of cgnr_host.stats_at, LSQR's
five scalars within max(1000·e, 1e-12).  tests/test_dist_iterates_host.py shows that a block normal
that misses a neighbour's rows, column norms from the owner's rows, a transfer that drops its entries
across a cut, λ from one slab's rows or a stale ghost ṽ each move x_k, k ≤ 3, by 1e9·τ_k and more.

CGNR, precond 3 and 1, k ∈ cgnr_host.KS on t64 and KS9 elsewhere (dist_host.CG_CASES):
    ksweep-7x70-8    2, 3, 4, 7 ranks   slabs of 4+3, 2+3+2, 2+2+1+2 rows and one row per rank; two x tiles
    ksweep-9x11-5    2, 4               a lattice narrower than one tile
    ksweep-5x200-13  2, 5               x tiles clear of both edges, 16-long register columns, one-row slabs
    t64              2, 3, 8            even cuts and odd ones (21, 43)
    t64-mask         3                  row mask, re-weighted data rows, warm start scattered to owned and
                                        ghost columns; once more after a plain-weights solve on the same handle
    t15              3                  15 epochs
    t64z             2, 3               z0 on a refined lattice: two lattices cut by one y bound
    ta64             3                  field-valued parts sliced per rank
  One-row slabs: the window kernels were read for a minimum height before these ran.  The column-mode
  ring (k_cg_normal_col, cg_strip) guards every staged row by 0 ≤ y < shape[0] and clips a strip to
  ye = min(ys + ty, shape[0]); windows of 2 or 3 rows give every row its own dim-0 class (ncls = shape);
  the wave-strip operator is not chosen below 8 rows per strip; k_blk_to_cols works block by block.
CGNR with multigrid (precond 4), k ∈ (1, 2, 3, 5, 8) (dist_host.MG_CASES): t64 with 2, 3, 4, 8 ranks,
  t64-mask with 3 (fresh, and after a plain-weights solve on the same handle), 33x33-5 with 2 (level 1
  partitioned by default), 7x70-8 with 2 and 3 (coarse levels replicated), 23x38-3 with 3 (level 1 the
  coarsest); in child processes LSQ_MG_PART_MIN=2 on 33x33-5 with 3 and 4 ranks and on t64 with 3, and
  LSQ_MG_PART=0 on t64 with 2.  The reference runs with the λ the ranks used (lsq_vgroup_mg_info), so
  λ and V fail separately; λ itself against mg_host.power_lambda within max(1000·e_λ, 1e-12).  Every rank
  reports the same λ and lp, and the ranks' [oa, ob) tile every level as the host restatement of the
  rule says.  33x33-5 has three levels (33, 17, 9 rows; the coarsest is never split), so its children
  have lp = 1, not the two partitioned levels one might expect from 33 → 17 → 9; t64 with 3 ranks has lp = 3.
LSQR over ranks (method 0, precond 0 and 1), windows and assembled ranks, k ∈ lsqr_host.K4 (t64: K):
  t64 with 2 and 3 ranks, t64-mask with 3, ksweep-9x11-5 with 4.  On structured ranks the ghost columns
  of a rank's own x come back exactly 0.
Refusal pinned: multigrid on t64z (the ranks cannot share one global lattice) raises NativeError.

Largest device / τ_k seen (profiles/dist_iterates.json, 64 entries): CGNR 0.073 (t64z, precond 3, 3 ranks;
every other system 0.044 and less, the one-row slabs 0.0021 to 0.0095), multigrid 0.028 (7x70-8, 2 ranks;
λ within 8e-4 of its tolerance), LSQR 0.016 (t64 windows, precond 1, 3 ranks; its scalars 0.0029 of
theirs); the CGNR estimates within 1.4e-12 of their definitions.  No case needed an explanation."""
import atexit
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the repository root on sys.path, also in the child process)
import cgnr_host as H
import dist_host as D
import lsqr_host as LH
import mg_host as M
from test_gpu_cgnr_iterates import EST, EST_TOL, Ref

pytestmark = pytest.mark.gpu
F64, LD = np.float64, np.longdouble
RECORD = {}


def _dump_record():
    path = os.environ.get('DIST_ITERATES_JSON')
    if path and RECORD:
        worst = {}
        for tag, rec in RECORD.items():
            fam = tag.split('/')[0]
            r = max((v['ratio'] for v in rec.values() if isinstance(v, dict) and 'ratio' in v), default=0.0)
            if r >= worst.get(fam, (0.0, ''))[0]:
                worst[fam] = (r, tag)
        out = dict(RECORD, largest={f: dict(ratio=r, case=t) for f, (r, t) in worst.items()})
        with open(path, 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)


atexit.register(_dump_record)


def _open(name, nranks, structured=True):
    from lssurf_amd import dist
    h = D.inputs(name)[0]
    return dist.VirtualDistFitSystem(h.S['G_data'], h.S['Gc'], h.keep_cols, h.n_full, nranks, structured=structured)


def _solves(vd, name, ks, precond, method, warm=True):
    """{k: (x_k, stats)} of the case's weights, mask and warm start on an open group: the weights go
    down once, then only maxit stops each solve"""
    h, w, mask, x0 = D.inputs(name)
    vd.set_row_mask(mask)
    out = {}
    for i, k in enumerate(ks):
        x = vd.solve(w if i == 0 else None, h.rhs if i == 0 else None, atol=0.0, btol=0.0, conlim=0.0 if method == 0 else 1e8,
                     maxit=k, precond=precond, method=method, x0=x0 if (warm and method == 1) else None)
        st = vd.stats
        assert st['method'] == method and st['istop'] == 7 and st['iters'] == k, (name, precond, k, st)
        out[k] = (x, st)
    return out


def _check_x(tag, what, dev, ref_x, e, tau):
    """x_k of {k: (x, stats)} within τ_k of ref_x[k]; the figures into RECORD; the failures returned"""
    rec = RECORD.setdefault(tag, {})
    bad = []
    for k, (x, _) in sorted(dev.items()):
        d = H.rel(np.asarray(x).astype(LD), ref_x[k])
        rec[str(k)] = dict(device=d, e_k=e[k], tau_k=tau[k], ratio=d / tau[k])
        print(f'{tag} k={k}: device {d:.2e}, e_k {e[k]:.2e}, tau_k {tau[k]:.2e}, ratio {d / tau[k]:.3g}')
        if not d <= tau[k]:
            bad.append(f'{what} k={k}: {d / tau[k]:.3g} tau_k (device {d:.3e}, tau_k {tau[k]:.3e})')
        assert np.all(np.isfinite(x)) and np.any(x != 0.0), (what, k)
    return bad


# ---- CGNR with block-Jacobi and Jacobi -----------------------------------------------------------------
def _cg_ks(name):
    return H.KS if name == 't64' else H.KS9


@functools.lru_cache(maxsize=None)
def _cg_ref(name, precond):
    h, _, _, x0 = D.inputs(name)
    A, b = D.system(name)
    f = H.block_factors(A, D.blocks(h)) if precond == 3 else H.jacobi_factors(A)
    return Ref(A, b, f, max(_cg_ks(name)), x0=x0)


def _check_cg(tag, what, dev, ref):
    bad = _check_x(tag, what, dev, ref.ld['x'], ref.e, ref.tau)
    worst = 0.0
    for k, (_, st) in sorted(dev.items()):
        want = ref.stats(k)
        for f in EST:
            err = abs(st[f] - want[f]) / want[f]
            worst = max(worst, err)
            if not err <= EST_TOL:
                bad.append(f'{what} k={k} {f}: {err:.3e} (device {st[f]!r}, host {want[f]!r})')
    RECORD[tag]['estimates_worst'] = worst
    print(f'{tag}: estimates within {worst:.2e}')
    return bad


CG_PARAMS = [(n, r) for n, by in D.CG_CASES.items() for r in by]


@pytest.mark.parametrize('name,nranks', CG_PARAMS, ids=[f'{n}-{r}' for n, r in CG_PARAMS])
def test_cgnr_iterates_match_host_reference(gpu_available, name, nranks):
    bad = []
    vd = _open(name, nranks)
    try:
        assert vd.has_blocks
        dev = {p: _solves(vd, name, _cg_ks(name), p, 1) for p in (3, 1)}
    finally:
        vd.close()
    for p in (3, 1):
        bad += _check_cg(f'cgnr/{name}/p{p}/r{nranks}', f'{name} precond {p} ranks {nranks}', dev[p], _cg_ref(name, p))
    assert not bad, bad


def test_cgnr_reweight_on_one_handle(gpu_available):
    """A solve with plain weights and every row kept, then the t64-mask iterates on the same group: block
    factors, column norms or ghost copies left from the first weights would show."""
    bad = []
    vd = _open('t64', 3)
    try:
        for p in (3, 1):
            _solves(vd, 't64', (5,), p, 1)
        dev = {p: _solves(vd, 't64-mask', H.KS9, p, 1) for p in (3, 1)}
    finally:
        vd.close()
    for p in (3, 1):
        bad += _check_cg(f'cgnr/t64-mask-after-plain/p{p}/r3', f't64-mask after plain weights precond {p} ranks 3', dev[p],
                         _cg_ref('t64-mask', p))
    assert not bad, bad


# ---- CGNR with multigrid ----------------------------------------------------------------------------
class MgRef:
    """One system's host hierarchy, the mirror's λ in both precisions, and per λ the PCG iterates."""

    def __init__(self, name):
        self.name = name
        self.h, _, _, self.x0 = D.inputs(name)
        self.A, self.b = D.system(name)
        self.S = M.case_system(name, self.A)
        self.rows = [lv[0][0] for lv in self.S.lev[F64]]
        self.lam64, self.lamld = self.S.host_lambda(F64), self.S.host_lambda(LD)

    @functools.lru_cache(maxsize=None)
    def iterates(self, lam):
        """(x_k in extended precision, e_k, τ_k) with the host cycle at the λ given (a tuple)"""
        xs = {dt: M.pcg_v(self.A, self.b, self.S.compact(self.S.cycle(list(lam), dt)), max(D.MG_KS), x0=self.x0, dtype=dt)
              for dt in (F64, LD)}
        e = {k: H.rel(xs[F64][k].astype(LD), xs[LD][k]) for k in D.MG_KS}
        return xs[LD], e, {k: max(1000 * v, 1e-13) for k, v in e.items()}

    def check_lambda(self, tag, what, lam):
        bad = []
        for l, (a, b, c) in enumerate(zip(lam, self.lam64, self.lamld)):
            e = float(abs(b - c) / c)
            tol = max(1000 * e, 1e-12)
            d = float(abs(LD(a) - c) / c)
            RECORD.setdefault(tag, {})[f'lambda{l}'] = dict(device_lambda=float(a), host_lambda=float(b), deviation=d, tol=tol)
            print(f'{tag} λ level {l}: device {a!r}, host {float(b)!r}, deviation {d:.2e}, tol {tol:.2e}')
            if not d <= tol:
                bad.append(f'{what} λ level {l}: {d / tol:.3g} tol (device {a!r}, host {float(b)!r})')
        return bad


@functools.lru_cache(maxsize=None)
def _mg_ref(name):
    return MgRef(name)


def _mg_infos(vd, nranks):
    return [vd.mg_info(r) for r in range(nranks)]


def _check_mg(tag, what, name, nranks, xs, infos, pmin=D.MG_PART_MIN, on=True, lp_least=None):
    """the ranks' accounts of their hierarchy, λ against the mirror, x_k against PCG with the host cycle"""
    ref = _mg_ref(name)
    L = len(ref.rows)
    for r, info in enumerate(infos):
        assert info['levels'] == L, (what, r, info)
        assert info['lp'] == infos[0]['lp'] and np.array_equal(info['lam'], infos[0]['lam']), (what, r, info, infos[0])
    bounds = [0] + [int(v) for v in np.cumsum(D.owned_rows(name, nranks))]
    lp_host, own = D.mg_partition(ref.rows[0], bounds, ref.rows, pmin, on)
    lp = infos[0]['lp']
    RECORD.setdefault(tag, {})['lp'] = lp
    for l in range(L):                     # [oa, ob) of every level: the host restatement, so no gap and no overlap
        got = [(int(info['oa'][l]), int(info['ob'][l])) for info in infos]
        assert got == own[l], (what, l, got, own[l])
        assert got[0][0] == 0 and got[-1][1] == ref.rows[l] and all(a[1] == b[0] for a, b in zip(got, got[1:]))
    assert lp <= lp_host, (what, lp, lp_host)              # never below LSQ_MG_PART_MIN rows, never the coarsest
    assert lp >= (min(lp_host, 1) if lp_least is None else lp_least), (what, lp, lp_host)
    lam = [float(v) for v in infos[0]['lam'][:L - 1]]
    assert infos[0]['lam'][L - 1] == 0.0 and min(lam) > 0
    bad = ref.check_lambda(tag, what, lam)
    ref_x, e, tau = ref.iterates(tuple(lam))
    bad += _check_x(tag, what, xs, ref_x, e, tau)
    return bad, lp


def _mg_run(name, nranks, after_plain=False):
    """({k: (x_k, stats)}, the ranks' mg_info after the first solve)"""
    from lssurf_amd._native import NativeError
    vd = _open(name, nranks)
    try:
        assert vd.has_blocks and vd.has_global
        with pytest.raises(NativeError, match='no multigrid solve'):
            vd.mg_info(0)
        if after_plain:
            base = name[:-5]
            _solves(vd, base, (3,), 4, 1)
            plain = _mg_infos(vd, nranks)
        dev = _solves(vd, name, D.MG_KS[:1], 4, 1)
        first = _mg_infos(vd, nranks)
        dev.update(_solves(vd, name, D.MG_KS[1:], 4, 1))
        last = _mg_infos(vd, nranks)
        with pytest.raises(NativeError, match='rank out of range'):
            vd.mg_info(nranks)
    finally:
        vd.close()
    for a, b in zip(first, last):          # the set-up of every solve gives the same λ for the same weights
        assert np.array_equal(a['lam'], b['lam']) and a['lp'] == b['lp']
    if after_plain:                        # and another λ for other weights
        assert not np.array_equal(plain[0]['lam'], first[0]['lam'])
    return dev, first


MG_PARAMS = [(n, r, False) for n, by in D.MG_CASES.items() for r in by] + [('t64-mask', 3, True)]


@pytest.mark.parametrize('name,nranks,after_plain', MG_PARAMS,
                         ids=[f'{n}-{r}' + ('-after-plain' if a else '') for n, r, a in MG_PARAMS])
def test_multigrid_iterates_match_host_reference(gpu_available, name, nranks, after_plain):
    dev, infos = _mg_run(name, nranks, after_plain)
    tag = f'mg/{name}{"-after-plain" if after_plain else ""}/r{nranks}'
    bad, _ = _check_mg(tag, f'{name} precond 4 ranks {nranks}', name, nranks, dev, infos)
    assert not bad, bad


# switches read once per process: fresh child processes, no device handle open here beside them
# tag -> the least lp the child must report (33x33-5: its 17-row level 1 is the only one that can be split)
CHILD_LP = {'33x33-5/3/min2': 1, '33x33-5/4/min2': 1, 't64/3/min2': 2, 't64/2/part0': 0}


@pytest.mark.parametrize('tag', list(D.MG_CHILDREN), ids=[t.replace('/', '-') for t in D.MG_CHILDREN])
def test_multigrid_partition_switches_in_child_processes(gpu_available, tmp_path, tag):
    name, nranks, env_extra = D.MG_CHILDREN[tag]
    _mg_ref(name)
    out = tmp_path / 'child.npz'
    env = dict(os.environ, **env_extra)
    for var in ('LSQ_MG_PART', 'LSQ_MG_PART_MIN', 'LSQ_MG_DEG', 'LSQ_MG_DEG0', 'LSQ_MG_DEG0_PRE', 'LSQ_MG_POW'):
        if var not in env_extra:
            env.pop(var, None)
    env.pop('DIST_ITERATES_JSON', None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(out), name, str(nranks)], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(out)
    infos = [dict(levels=int(got['levels']), lp=int(got['lp'][q]), lam=got['lam'][q], oa=got['oa'][q], ob=got['ob'][q])
             for q in range(nranks)]
    xs = {k: (got[f'x{k}'], None) for k in D.MG_KS}
    on = env_extra.get('LSQ_MG_PART') != '0'
    bad, lp = _check_mg(f'mg/{tag}', f'{tag} precond 4', name, nranks, xs, infos,
                        pmin=int(env_extra.get('LSQ_MG_PART_MIN', D.MG_PART_MIN)), on=on, lp_least=CHILD_LP[tag])
    if not on:
        assert lp == 0
    assert not bad, bad


def _child(path, name, nranks):
    dev, infos = _mg_run(name, nranks)
    np.savez(path, levels=infos[0]['levels'], lp=[i['lp'] for i in infos], lam=[i['lam'] for i in infos],
             oa=[i['oa'] for i in infos], ob=[i['ob'] for i in infos], **{f'x{k}': x for k, (x, _) in dev.items()})


def test_multigrid_refuses_two_lattices(gpu_available):
    """t64z: z0 on a refined lattice, so the ranks have no one global lattice to describe
    (lsq_dist_set_global is not installed) and precond 4 says so; precond 3 and 1 run (the CGNR cases)."""
    from lssurf_amd._native import NativeError
    h, w, _, _ = D.inputs('t64z')
    vd = _open('t64z', 2)
    try:
        assert vd.has_blocks and not vd.has_global
        with pytest.raises(NativeError, match='lsq_dist_set_global'):
            vd.solve(w, h.rhs, atol=0.0, btol=0.0, maxit=1, precond=4, method=1)
    finally:
        vd.close()


# ---- LSQR over ranks ---------------------------------------------------------------------------------
LSQR_PARAMS = [(n, r, s) for n, by in D.LSQR_CASES.items() for r in by for s in (True, False)]


@pytest.mark.parametrize('name,nranks,structured', LSQR_PARAMS,
                         ids=[f'{n}-{r}-{"windows" if s else "assembled"}' for n, r, s in LSQR_PARAMS])
def test_lsqr_iterates_match_host_reference(gpu_available, name, nranks, structured):
    ks = LH.K if name == 't64' else LH.K4
    c = LH.case(name)
    h, w, mask, _ = D.inputs(name)
    assert c.h is h and np.array_equal(c.w, w) and np.array_equal(c.mask, mask) and c.x0 is None
    vd = _open(name, nranks, structured)
    dev = {}
    try:
        for p in (0, 1):
            dev[p] = _solves(vd, name, ks, p, 0, warm=False)
            if structured:                 # a rank's ghost columns carry no column scale: exactly 0 in its own x
                for prob, xl in zip(vd.probs, vd.x_local):
                    own = np.zeros(prob['n_full'], bool)
                    for a, b in prob['own_ranges']:
                        own[a:b] = True
                    ghost = ~own[prob['keep']]
                    assert ghost.any() and np.all(xl[ghost] == 0.0) and np.any(xl[~ghost] != 0.0)
    finally:
        vd.close()
    bad = []
    for p in (0, 1):
        ref = c.ref(p, max(ks))
        kind = 'windows' if structured else 'assembled'
        tag, what = f'lsqr/{name}/{kind}/p{p}/r{nranks}', f'{name} LSQR precond {p} {kind} ranks {nranks}'
        bad += _check_x(tag, what, dev[p], ref.ld['x'], ref.e, ref.tau)
        worst = 0.0
        for k, (_, st) in sorted(dev[p].items()):
            for f in LH.SCALARS:
                ds = ref.sdev(f, k, st[f])
                worst = max(worst, ds / ref.taus[f][k])
                if not ds <= ref.taus[f][k]:
                    bad.append(f'{what} k={k} {f}: {ds / ref.taus[f][k]:.3g} tau (device {st[f]!r}, host {float(ref.ld[f][k])!r})')
        RECORD[tag]['scalars_worst_ratio'] = worst
        print(f'{tag}: scalars within {worst:.3g} of their tolerance')
    assert not bad, bad


if __name__ == '__main__':
    if len(sys.argv) == 5 and sys.argv[1] == '--child':
        _child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
