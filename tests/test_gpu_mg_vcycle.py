"""The multigrid V-cycle (lsq precond 4; lssurf_amd/csrc/mg.inc) against the host cycle of
tests/mg_host.py: the same levels (already pinned operator by operator elsewhere), the node-block
factors rounded to bf16 as the device rounds them, Chebyshev smoothing, restriction, prolongation
and the coarsest solve written from the definitions and run in extended precision.

1. λ of every smoothing level (mg_apply(l, 2)) equals the host mirror of the set-up's power steps
   (hashed start vector, M-normalised iterates) within max(1000·e_λ, 1e-12), e_λ the mirror's own
   float64-against-extended spread: the first check of the operator kernels' pold / β / pnew path.
2. Coverage: λ_max(M̃⁻¹N_ℓ) (Lanczos on the host) < 1.21·λ_dev.  The smoother's interval is
   [0.11 λ, 1.1 λ]; a Chebyshev polynomial on it stops contracting at eigenvalues above
   2θ = 1.21 λ (|T_k(y)| < T_k(σ) ⇔ |y| < σ).
3. V(u) from level 0 and 4. from every coarser level (the coarsest: its dense inverse) equal the host
   cycle run with the DEVICE's λ (so 1 and 3 fail separately) within τ = max(1000·e_V, 1e-13) of the
   extended-precision result, e_V the host's float64-against-extended spread (the rule of
   tests/test_gpu_cgnr_iterates.py); removed columns exactly 0.  A failure names its level.
5. The same with LSQ_MG_DEG0=3, LSQ_MG_DEG=2: the steps that read and store the direction d.
6. t64 in child processes with the level operators forced onto the ring (LSQ_MG_DIRECT=0) and the
   tile kernels (… LSQ_MG_TILE=1): same λ and V(u).
7. PCG iterates x_k, k ∈ {1, 2, 3, 5, 8} (zero tolerances: only maxit stops the solve) against
   textbook PCG with the host cycle, τ_k = max(1000·e_k, 1e-13); in child processes every
   LSQ_MG_FUSE ∈ {0, 1, 4, 5}: the CG update's fused first smoothing step (bit 0), the restriction
   fused into the next smoother (bit 2), ρ from the last smoother's partials.

Both host precisions run on the same float64 level operators, so e_V (1e-16 … 2e-14) is their
arithmetic alone; the defects of tests/test_mg_host.py's sensitivity test move V(u) by 7e-4 and more.
t64z (z0 on a refined lattice: the mgx_* kernels) exposes its fine level only, so its dz-lattice
levels run with the mirror's λ.

Every case runs its device calls BEFORE get_csr() (tests/test_gpu_cgnr_iterates.py explains).  The
figures go to the file named by MG_VCYCLE_JSON, when set (profiles/mg_vcycle.json is one such run)."""
import atexit
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the repository root on sys.path, also in the child process)
import cgnr_host as CH
import mg_host as M
from test_gpu_cgnr_iterates import _env, _same_as_host

pytestmark = pytest.mark.gpu
F64, LD = np.float64, np.longdouble
KS = (1, 2, 3, 5, 8)
ZERO = dict(atol=0.0, btol=0.0, method=1, precond=4)
PCG_CASES = ['t64', 't64-mask', '7x70-8', 't64z']
SAME_LATTICE = [n for n in M.CASES if n != 't64z']      # a z0-refined system exposes its fine level only
COVER = 1.21

RECORD = {}


def _short(v):
    """deviations to three digits, ratios to four decimals, the λ values as they are"""
    if isinstance(v, dict):
        return {k: (x if k in ('device_lambda', 'host_lambda') else _short(x)) for k, x in v.items()}
    return (round(v, 4) if v >= 0.1 else float(f'{v:.3g}')) if isinstance(v, float) else v


def _dump_record():
    """one line per figure; a tag whose figures equal an earlier tag's names that tag instead"""
    path = os.environ.get('MG_VCYCLE_JSON')
    if not (path and RECORD):
        return
    rec, tags = {t: _short(RECORD[t]) for t in RECORD}, []
    for t in sorted(rec):
        same = next((o for o in sorted(rec) if o < t and rec[o] == rec[t]), None)
        if same:
            tags.append(f' {json.dumps(t)}: {{"same_as": {json.dumps(same)}}}')
            continue
        kinds = []
        for kind in sorted(rec[t]):
            rows = ',\n'.join(f'   {json.dumps(k)}: {json.dumps(v, sort_keys=True)}' for k, v in sorted(rec[t][kind].items()))
            kinds.append(f'  {json.dumps(kind)}: {{\n{rows}\n  }}')
        tags.append(f' {json.dumps(t)}: {{\n' + ',\n'.join(kinds) + '\n }')
    with open(path, 'w') as f:
        f.write('{\n' + ',\n'.join(tags) + '\n}\n')


atexit.register(_dump_record)


def _is_mixed(h):
    return tuple(h.S['grids']['z0'].shape) != tuple(h.S['grids']['dz'].shape[:2])


def _level_keeps(h, levels, nt):
    """the kept-column mask of every level's full column space, from mg_info's lattices"""
    nn = levels[0][0] * levels[0][1]
    keep0 = np.zeros(levels[0][2], bool)
    keep0[h.keep_cols] = True
    if _is_mixed(h):                    # z0 on a refined lattice: the fine level only
        return [keep0]
    kt = keep0[nn:nn + nt]
    out = [keep0]
    for S0, S1, nf in levels[1:]:
        out.append(np.concatenate([np.ones(S0 * S1, bool), np.tile(kt, S0 * S1)]))
        assert out[-1].size == nf
    return out


def _x0(name, h):
    return CH.warm_start(h) if name == 't64-mask' else None


def _device(name, ks=(), coarse_v=True):
    """The device's side of a case: λ per smoothing level, V_l(u) of two vectors per level, x_k of a
    solve stopped at maxit = k; then the formed A.  One FitSystem, closed before returning."""
    h, w, mask, (ny, nx, nt) = M.case_host(name)
    out = {}
    fs = h.fit_system()
    try:
        fs.solver.set_row_weight(w)
        fs.solver.set_row_mask(mask)
        ok, why = fs.solver.cg_available(4)
        assert ok, why
        levels, _ = fs.solver.mg_info()
        out['levels'] = levels
        keeps = _level_keeps(h, levels, nt)
        if len(keeps) > 1:
            out['family'] = np.array([fs.solver.mg_apply(l, 3) for l in range(len(levels))])
        out['lam'] = np.array([fs.solver.mg_apply(l, 2) for l in range(len(keeps) - 1 if len(keeps) > 1 else 1)])
        for l in range(len(keeps) if coarse_v else 1):
            for i, u in enumerate(M.test_vectors(keeps[l])):
                out[f'V{l}_{i}'] = fs.solver.mg_apply(l, 1, u)
        for k in ks:
            x, st = fs.solver.solve(h.rhs, x0=_x0(name, h), maxit=k, **ZERO)
            assert st['method'] == 1 and st['istop'] == 7 and st['iters'] == k, st
            out[f'x{k}'] = x
        out['A'] = fs.solver.get_csr()
    finally:
        fs.close()
    return out


class Ref:
    """The host references of one system (a mg_host.System built from the device's formed A) at the
    device's λ, and the comparisons against them."""

    def __init__(self, S, lam, **degrees):
        self.S, self.lam, self.levels = S, lam, S.lev[F64]
        self.V64, self.Vld = S.cycle(lam, F64, **degrees), S.cycle(lam, LD, **degrees)

    @functools.lru_cache(maxsize=None)
    def v_ref(self, l, i):
        """(V_ld(u), e_V, τ) of test vector i on level l"""
        u = M.test_vectors(self.levels[l][1])[i]
        ref = self.Vld(u, l)
        e = CH.rel(self.V64(u, l).astype(LD), ref)
        return ref, e, max(1000 * e, 1e-13)

    def check_v(self, tag, l, i, got):
        ref, e, tau = self.v_ref(l, i)
        d = CH.rel(np.asarray(got).astype(LD), ref)
        RECORD.setdefault(tag, {}).setdefault('V', {})[f'{l}/{i}'] = dict(device=d, e_V=e, tau=tau)
        print(f'{tag} V level {l} vector {i}: device {d:.2e}, e_V {e:.2e}, tau {tau:.2e}')
        assert np.all(np.asarray(got)[~self.levels[l][1]] == 0.0), (tag, l)
        return None if d <= tau else (l, i, d, tau)

    def check_lambda(self, tag, lam_dev):
        h64 = self.S.host_lambda(F64)
        hld = self.S.host_lambda(LD)
        bad = []
        for l, (a, b, c) in enumerate(zip(lam_dev, h64, hld)):
            e = float(abs(b - c) / c)
            tol = max(1000 * e, 1e-12)
            d = float(abs(LD(a) - c) / c)
            RECORD.setdefault(tag, {}).setdefault('lambda', {})[str(l)] = dict(device_lambda=float(a), host_lambda=float(b),
                                                                              deviation=d, e_lambda=e, tol=tol)
            print(f'{tag} λ level {l}: device {a!r}, host {float(b)!r}, deviation {d:.2e}, tol {tol:.2e}')
            if not d <= tol:
                bad.append((l, float(a), float(b), d, tol))
        assert not bad, (tag, bad)


class Case(Ref):
    """A case of mg_host.CASES: its device results beside the references."""

    def __init__(self, name, degs=None):
        self.name = name
        h, w, mask, _ = M.case_host(name)
        ks = KS if (name in PCG_CASES and degs is None) else ()
        if degs is None:
            self.dev = _device(name, ks)
        else:
            with _env('LSQ_MG_DEG0', str(degs[0])), _env('LSQ_MG_DEG', str(degs[1])):
                self.dev = _device(name, ks)
        A = self.dev.pop('A')
        _same_as_host(A, h.A(w, mask))
        self.h, self.A, self.b = h, A, (w * h.rhs)[mask]
        S = M.case_system(name, A)
        lam = [float(v) for v in self.dev['lam']]
        if name == 't64z':     # the dz-lattice levels' λ: the mirror's (test 1 pins it on every other case)
            lam += [float(v) for v in S.sub.host_lambda()]
        super().__init__(S, lam, **({} if degs is None else dict(deg0=degs[0], deg=degs[1])))
        assert [(s[0], s[1]) for s in self.dev['levels']] == [lv[0] for lv in self.levels]

    @functools.lru_cache(maxsize=None)
    def pcg_ref(self):
        """(x_k in extended precision, e_k, τ_k) of the case's solve"""
        x0 = _x0(self.name, self.h)
        xs = {dt: M.pcg_v(self.A, self.b, self.S.compact(V), max(KS), x0=x0, dtype=dt)
              for dt, V in ((F64, self.V64), (LD, self.Vld))}
        e = {k: CH.rel(xs[F64][k].astype(LD), xs[LD][k]) for k in KS}
        return xs[LD], e, {k: max(1000 * v, 1e-13) for k, v in e.items()}

    def check_x(self, tag, xs):
        ref, e, tau = self.pcg_ref()
        bad = []
        for k in KS:
            d = CH.rel(np.asarray(xs[k]).astype(LD), ref[k])
            RECORD.setdefault(tag, {}).setdefault('x', {})[str(k)] = dict(device=d, e_k=e[k], tau_k=tau[k])
            print(f'{tag} x_{k}: device {d:.2e}, e_k {e[k]:.2e}, tau_k {tau[k]:.2e}')
            if not d <= tau[k]:
                bad.append((k, d, tau[k]))
        assert not bad, (tag, bad)


@functools.lru_cache(maxsize=None)
def _case(name, degs=None):
    return Case(name, degs)


@pytest.mark.parametrize('name', M.CASES)
def test_lambda_matches_the_host_power_steps(gpu_available, name):
    c = _case(name)
    c.check_lambda(name, c.lam)


@pytest.mark.parametrize('name', M.CASES)
def test_smoothing_interval_covers_the_spectrum(gpu_available, name):
    c = _case(name)
    bad = []
    for l, lam in enumerate(c.lam):
        ratio = c.S.level_lambda_max(l) / lam
        RECORD.setdefault(name, {}).setdefault('coverage', {})[str(l)] = ratio
        print(f'{name} level {l}: λ_max / λ_dev = {ratio:.4f}')
        if not ratio < COVER:
            bad.append((l, ratio))
    assert not bad, (name, bad)


@pytest.mark.parametrize('name', M.CASES)
def test_vcycle_matches_host(gpu_available, name):
    c = _case(name)
    bad = [c.check_v(name, 0, i, c.dev[f'V0_{i}']) for i in range(2)]
    assert not any(bad), (name, bad)


@pytest.mark.parametrize('name', SAME_LATTICE)
def test_vcycle_from_every_level_matches_host(gpu_available, name):
    c = _case(name)
    bad = [c.check_v(name, l, i, c.dev[f'V{l}_{i}']) for l in range(1, len(c.levels)) for i in range(2)]
    assert not any(bad), (name, bad)


@pytest.mark.parametrize('name', ['t64', '7x70-8'])
def test_vcycle_degrees_3_and_2(gpu_available, name):
    """LSQ_MG_DEG0=3, LSQ_MG_DEG=2: MG_NEEDD on every level, d stored without MG_NOD on level 0"""
    c = _case(name, (3, 2))
    tag = f'{name}-deg32'
    bad = [c.check_v(tag, l, i, c.dev[f'V{l}_{i}']) for l in range(len(c.levels)) for i in range(2)]
    assert not any(bad), (tag, bad)


@pytest.mark.parametrize('name', PCG_CASES)
def test_pcg_iterates_match_host(gpu_available, name):
    c = _case(name)
    c.check_x(name, {k: c.dev[f'x{k}'] for k in KS})


def test_t256(gpu_available):
    """t256 (the benchmark's layout at a quarter of its size), once: λ and coverage of its six smoothing
    levels and V(u) from level 0.  Level 1 (216 k columns) runs the tile kernel k_mg_tile_kt, whose
    pold / β / pnew path only the power steps use (level 2, 55 k columns, is below MG_TILE_MIN: k_mg_direct);
    level 0 runs the ring kernel, the data-row kernels and the transfers over 786 k columns.  The factors' bf16 check of tests/test_mg_host.py runs here for this system."""
    h = CH.synthetic_host('t256')
    fs = h.fit_system()
    try:
        fs.solver.set_row_weight(h.w)
        fs.solver.set_row_mask(np.ones(h.w.size, bool))
        ok, why = fs.solver.cg_available(4)
        assert ok, why
        levels, _ = fs.solver.mg_info()
        family = [fs.solver.mg_apply(l, 3) for l in range(len(levels))]
        assert levels[1][2] > 1 << 16 and family[:3] == [0, 3, 1] and family[-1] == -1, family
        lam = [fs.solver.mg_apply(l, 2) for l in range(len(levels) - 1)]
        u = M.test_vectors(_level_keeps(h, levels, 12)[0], 1)[0]
        Vu = fs.solver.mg_apply(0, 1, u)
        A = fs.solver.get_csr()
    finally:
        fs.close()
    _same_as_host(A, h.A())
    S = M.System(A, h.n_data, h.keep_cols, (256, 256, 12))
    for l, f in enumerate(M.level_factors(S.lev[F64], S.nt, round=False)[:-1]):      # asserts the pivots
        assert CH.at_risk_entries(CH.factor_entries(f)) == 0, l
    c = Ref(S, lam)
    c.check_lambda('t256', lam)
    bad = []
    for l in range(len(lam)):
        ratio = S.level_lambda_max(l, 1e-5) / lam[l]
        RECORD.setdefault('t256', {}).setdefault('coverage', {})[str(l)] = ratio
        print(f't256 level {l}: λ_max / λ_dev = {ratio:.4f}')
        if not ratio < COVER:
            bad.append((l, ratio))
    assert not bad, bad
    assert c.check_v('t256', 0, 0, Vu) is None


# ---- switches read once per process: fresh child processes ----------------------------------------
def _child_run(tmp_path, tag, env_extra):
    out = tmp_path / f'{tag}.npz'
    env = dict(os.environ, **env_extra)
    for name in ('LSQ_MG_DEG', 'LSQ_MG_DEG0', 'LSQ_MG_DEG0_PRE', 'LSQ_MG_POW'):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(out)], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(out)


def _child(path):
    dev = _device('t64', KS, coarse_v=False)
    np.savez(path, **{k: v for k, v in dev.items() if k not in ('A', 'levels')})


CHILDREN = {'default': {}, 'ring': {'LSQ_MG_DIRECT': '0'}, 'tile': {'LSQ_MG_DIRECT': '0', 'LSQ_MG_TILE': '1'},
            'fuse0': {'LSQ_MG_FUSE': '0'}, 'fuse1': {'LSQ_MG_FUSE': '1'}, 'fuse4': {'LSQ_MG_FUSE': '4'},
            'fuse5': {'LSQ_MG_FUSE': '5'}}


@pytest.mark.parametrize('which', list(CHILDREN))
def test_kernel_families_and_fusions_in_child_processes(gpu_available, tmp_path, which):
    """λ, V(u) and the PCG iterates of t64 under each switch (6 and 7 of the list above), against the
    same host numbers as the in-process t64 case."""
    c = _case('t64')                      # its FitSystem is closed: no device handle open beside the child
    got = _child_run(tmp_path, which, CHILDREN[which])
    tag = f't64-{which}'
    family = [int(v) for v in got['family']]             # per level: 0 ring, 1 direct, 2 / 3 tile, −1 coarsest
    if which == 'ring':
        assert family == [0, 0, 0, 0, -1], family
    elif which == 'tile':
        assert family[0] == 0 and family[1] >= 2 and 1 not in family, family
    else:
        assert family == [0, 1, 1, 1, -1], family
    c.check_lambda(tag, got['lam'])
    # the host cycle runs with the in-process λ: a child whose λ passed differs from it by rounding
    bad = [c.check_v(tag, 0, i, got[f'V0_{i}']) for i in range(2)]
    assert not any(bad), (tag, bad)
    c.check_x(tag, {k: got[f'x{k}'] for k in KS})


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--child':
        _child(sys.argv[2])
