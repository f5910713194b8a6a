"""Robust spread and the extra data error used by smooth_fit's outlier editing.

Mirror of LSsurf/RDE.py:10-18 and LSsurf/calc_sigma_extra.py:13-109.  With `device` set, the
25–30 RDE evaluations of calc_sigma_extra's bounded search sort on the GPU (liblsqsurf
lsq_rde_*): r and σ are uploaded once per group, each evaluation
returns only the four order statistics numpy's interpolation needs, and the interpolation and
scipy's bounded Brent search run unchanged on the host — the result is bit-identical to the
host path (tests/test_gpu_smooth_fit.py).  The binned mode (calc_sigma_extra_on_grid) and several
groups run every (bin × group) search together: the selections become index segments, scipy's
bounded search is ported as a generator (_bounded_search) and all searches advance one evaluation
per call of a segmented evaluator — liblsqsurf's radix select (DeviceSelect, lsq_rde_select) or
np.sort (HostSelect) — again bit-identical to the per-bin host loop
(tests/test_sigma_extra_grid_host.py, tests/test_gpu_rde_select.py).
"""
import ctypes
import warnings

import numpy as np
import scipy.optimize as scipyo


def RDE(x):
    """Half the 16–84 percentile spread of the finite values (linear interpolation on
    mid-rank positions 0.5, 1.5, ...), NaN with fewer than two finite values."""
    finite = np.isfinite(x)
    n = int(np.sum(finite))
    if n < 2:
        return np.nan
    lo, hi = np.interp(np.array([0.16, 0.84]) * n, np.arange(0.5, n), np.sort(x[finite]))
    return (hi - lo) / 2.


class DeviceRDE:
    """RDE(r / sqrt(s² + σ²)) on the device for a fixed (r, σ); bit-identical to
    RDE(r / np.sqrt(s ** 2 + sigma ** 2)) on the host."""

    def __init__(self, r, sigma, device=0):
        from ._native import NativeError, load, ptr
        self._L, self._ptr = load(), ptr
        r = np.ascontiguousarray(r, dtype=np.float64)
        sigma = np.ascontiguousarray(sigma, dtype=np.float64)
        keep = np.isfinite(r) & np.isfinite(sigma)
        self.r, self.sigma = r[keep], sigma[keep]
        self.n = int(self.r.size)
        self._c = None
        if self.n >= 2:
            self._c = self._L.lsq_rde_create(int(device), self.n, ptr(self.r), ptr(self.sigma))
            if not self._c:
                raise NativeError('lsq_rde_create failed (no gfx950 device?)')

    def __call__(self, s):
        n = self.n
        if n < 2 or not np.isfinite(s):
            return RDE(self.r / np.sqrt(s ** 2 + self.sigma ** 2))   # degenerate: host path
        q = np.array([0.16, 0.84]) * n
        j = np.clip(np.floor(q - 0.5).astype(np.int64), 0, n - 2)
        idx = np.ascontiguousarray(np.stack([j, j + 1], axis=1).ravel(), dtype=np.int64)
        v = np.zeros(4)
        if self._L.lsq_rde_order_stats(self._c, float(s), 4, self._ptr(idx), self._ptr(v)) != 0:
            from ._native import NativeError
            raise NativeError(self._L.lsq_rde_last_error(self._c).decode())
        # np.interp on the two bracketing mid-rank positions = np.interp on all of them
        lo = np.interp(q[0], j[0] + np.array([0.5, 1.5]), v[0:2])
        hi = np.interp(q[1], j[1] + np.array([0.5, 1.5]), v[2:4])
        return (hi - lo) / 2.

    def close(self):
        if self._c:
            self._L.lsq_rde_destroy(self._c)
            self._c = None

    def __del__(self):
        self.close()


# ---- many (bin × group) segments at once: lock-step search over a segmented select -------------

def _bounded_search(x1, x2, xatol=1e-5, maxiter=500):
    """scipy.optimize.minimize_scalar(method='bounded') (scipy 1.15 _minimize_scalar_bounded,
    default options) as a generator: it yields the next abscissa and is sent the function value
    there; its return value (StopIteration.value) is (x, nfev).  The statements, their order and
    their scalar types are scipy's, so x is bit-identical; every loop turn makes exactly one
    evaluation, which is what lets many searches advance together."""
    if not (np.size(x1) == 1 and np.isfinite(x1) and np.size(x2) == 1 and np.isfinite(x2)):
        raise ValueError("Optimization bounds must be finite scalars.")
    if x1 > x2:
        raise ValueError("The lower bound exceeds the upper bound.")
    maxfun = maxiter
    sqrt_eps = np.sqrt(2.2e-16)
    golden_mean = 0.5 * (3.0 - np.sqrt(5.0))
    a, b = x1, x2
    fulc = a + golden_mean * (b - a)
    nfc, xf = fulc, fulc
    rat = e = 0.0
    x = xf
    fx = yield x
    num = 1
    ffulc = fnfc = fx
    xm = 0.5 * (a + b)
    tol1 = sqrt_eps * np.abs(xf) + xatol / 3.0
    tol2 = 2.0 * tol1
    while (np.abs(xf - xm) > (tol2 - 0.5 * (b - a))):
        golden = 1
        # Check for parabolic fit
        if np.abs(e) > tol1:
            golden = 0
            r = (xf - nfc) * (fx - ffulc)
            q = (xf - fulc) * (fx - fnfc)
            p = (xf - fulc) * q - (xf - nfc) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = np.abs(q)
            r = e
            e = rat
            # Check for acceptability of parabola
            if ((np.abs(p) < np.abs(0.5 * q * r)) and (p > q * (a - xf)) and
                    (p < q * (b - xf))):
                rat = (p + 0.0) / q
                x = xf + rat
                if ((x - a) < tol2) or ((b - x) < tol2):
                    si = np.sign(xm - xf) + ((xm - xf) == 0)
                    rat = tol1 * si
            else:      # do a golden-section step
                golden = 1
        if golden:  # do a golden-section step
            if xf >= xm:
                e = a - xf
            else:
                e = b - xf
            rat = golden_mean * e
        si = np.sign(rat) + (rat == 0)
        x = xf + si * np.maximum(np.abs(rat), tol1)
        fu = yield x
        num += 1
        if fu <= fx:
            if x >= xf:
                a = xf
            else:
                b = xf
            fulc, ffulc = nfc, fnfc
            nfc, fnfc = xf, fx
            xf, fx = x, fu
        else:
            if x < xf:
                a = x
            else:
                b = x
            if (fu <= fnfc) or (nfc == xf):
                fulc, ffulc = nfc, fnfc
                nfc, fnfc = x, fu
            elif (fu <= ffulc) or (fulc == xf) or (fulc == nfc):
                fulc, ffulc = x, fu
        xm = 0.5 * (a + b)
        tol1 = sqrt_eps * np.abs(xf) + xatol / 3.0
        tol2 = 2.0 * tol1
        if num >= maxfun:
            break
    return xf, num


def _segment_ranks(n):
    """The two percentile positions of RDE over n values and the 0-based ranks bracketing them
    (j_lo, j_lo+1, j_hi, j_hi+1), as DeviceRDE.__call__ computes them."""
    q = np.array([0.16, 0.84]) * n
    j = np.clip(np.floor(q - 0.5).astype(np.int64), 0, n - 2)
    return q, j


def _rde_of_stats(q, j, v):
    # np.interp on the two bracketing mid-rank positions = np.interp on all of them
    lo = np.interp(q[0], j[0] + np.array([0.5, 1.5]), v[0:2])
    hi = np.interp(q[1], j[1] + np.array([0.5, 1.5]), v[2:4])
    return (hi - lo) / 2.


class HostSelect:
    """The four order statistics per segment by np.sort on the host (the reference evaluator of
    the batched path, and the check of DeviceSelect)."""

    def __init__(self, r, sigma, seg_ptr, seg_idx, seg_rank):
        self.r, self.sigma, self.ptr, self.idx, self.rank = r, sigma, seg_ptr, seg_idx, seg_rank

    def __call__(self, seg, s, raw=False):
        out = np.zeros((len(seg), 4))
        for a, k in enumerate(seg):
            idx = self.idx[self.ptr[k]:self.ptr[k + 1]]
            rr = self.r[idx]
            x = rr if raw else rr / np.sqrt(s[a] ** 2 + self.sigma[idx] ** 2)
            out[a] = np.sort(x)[self.rank[k]]
        return out

    def close(self):
        pass


class DeviceSelect:
    """The same on the device: liblsqsurf's segmented radix select (lsq_rde_create_segments /
    lsq_rde_select), one call per evaluation of all active segments."""

    def __init__(self, r, sigma, seg_ptr, seg_idx, seg_rank, device=0):
        from ._native import NativeError, NativeRefused, load, ptr
        self._L, self._p = load(), ptr
        self.r = np.ascontiguousarray(r, dtype=np.float64)
        self.sigma = np.ascontiguousarray(sigma, dtype=np.float64)
        self.ptr = np.ascontiguousarray(seg_ptr, dtype=np.int64)
        self.idx = np.ascontiguousarray(seg_idx, dtype=np.int32)
        self.rank = np.ascontiguousarray(seg_rank, dtype=np.int64).reshape(-1, 4)
        self._c = None
        status = ctypes.c_int(0)
        c = self._L.lsq_rde_create_segments(int(device), self.r.size, ptr(self.r), ptr(self.sigma),
                                            self.ptr.size - 1, ptr(self.ptr), ptr(self.idx), ptr(self.rank),
                                            ctypes.byref(status))
        if not c:
            msg = self._L.lsq_rde_last_error(None).decode()
            raise (NativeRefused if status.value == -5 else NativeError)(
                f'lsq_rde_create_segments failed ({status.value}): {msg}')
        self._c = c

    def __call__(self, seg, s, raw=False):
        seg = np.ascontiguousarray(seg, dtype=np.int32)
        s = np.ascontiguousarray(s, dtype=np.float64)
        out = np.zeros((seg.size, 4))
        rc = self._L.lsq_rde_select(self._c, seg.size, self._p(seg), self._p(s), int(bool(raw)), self._p(out))
        if rc != 0:
            from ._native import NativeError
            raise NativeError(f'lsq_rde_select failed ({rc}): ' + self._L.lsq_rde_last_error(self._c).decode())
        return out

    def close(self):
        if self._c:
            self._L.lsq_rde_destroy(self._c)
            self._c = None

    def __del__(self):
        self.close()


def _refused():
    from ._native import NativeRefused
    return NativeRefused


def _evaluator_for(evaluator, device):
    """'host' / 'device' / a callable (r, sigma, seg_ptr, seg_idx, seg_rank) -> evaluator object;
    None: the device one when `device` is set."""
    if callable(evaluator):
        return evaluator
    if evaluator == 'host' or (evaluator is None and device is None):
        return HostSelect
    if evaluator in (None, 'device'):
        return lambda *a: DeviceSelect(*a, device=0 if device is None else device)
    raise ValueError(f'unknown evaluator {evaluator!r}')


def _batch_ok(r, sigma, mask, groups):
    """The batched path assumes every scaled residual is finite (as DeviceRDE does)."""
    sel = mask & np.logical_or.reduce(groups) if groups else mask
    rr, ss = r[sel], sigma[sel]
    return bool(np.all(np.isfinite(rr)) and np.all(np.isfinite(ss)) and np.all(ss != 0))


def _search_segments(r, sigma, segs, make_eval):
    """calc_sigma_extra's search for every index list in `segs` (each >= 2 points) at once: the
    upper bound RDE(r) from a raw select, then scipy's bounded search per segment as a state
    machine, all segments advancing one evaluation per evaluator call and dropping out as they
    finish.  Returns one value per segment (None where the search raised: the reference prints
    and continues)."""
    S = len(segs)
    if S == 0:
        return []
    seg_ptr = np.zeros(S + 1, dtype=np.int64)
    np.cumsum([idx.size for idx in segs], out=seg_ptr[1:])
    seg_idx = np.concatenate(segs).astype(np.int32)
    qs, js = zip(*[_segment_ranks(idx.size) for idx in segs])
    seg_rank = np.stack([np.stack([j, j + 1], axis=1).ravel() for j in js])
    ev = make_eval(r, sigma, seg_ptr, seg_idx, seg_rank)
    try:
        v = ev(np.arange(S), np.zeros(S), raw=True)
        result, gens, xs = [None] * S, {}, {}
        for k in range(S):
            try:
                gens[k] = _bounded_search(0, _rde_of_stats(qs[k], js[k], v[k]))
                xs[k] = next(gens[k])
            except Exception as err:   # the reference prints and continues
                print(err)
                gens.pop(k, None)
        while gens:
            active = list(gens)
            v = ev(np.array(active), np.array([float(xs[k]) for k in active]))
            for a, k in enumerate(active):
                try:
                    xs[k] = gens[k].send((_rde_of_stats(qs[k], js[k], v[a]) - 1) ** 2)
                except StopIteration as stop:
                    result[k] = stop.value[0]
                    del gens[k]
                except Exception as err:
                    print(err)
                    del gens[k]
        return result
    finally:
        ev.close()


def calc_sigma_extra(r, sigma, mask, sigma_extra_masks=None, device=None, evaluator=None):
    """sigma_extra such that RDE(r / sqrt(sigma² + sigma_extra²)) == 1 (bounded scalar search
    on [0, RDE(r)]), per sigma_extra mask; groups with < 10 selected points get 0.  With
    `device` (GPU ordinal) the RDE evaluations run on the device (same result): one group sorts
    there (DeviceRDE), several groups — or `evaluator` ('host' / 'device') — search in lock-step
    over the segmented select (_search_segments)."""
    if sigma_extra_masks is None:
        sigma_extra_masks = {'all': np.ones_like(r, dtype=bool)}
    if evaluator is not None or (device is not None and len(sigma_extra_masks) > 1):
        groups = [np.asarray(g, dtype=bool) for g in sigma_extra_masks.values()]
        mask_b = np.asarray(mask, dtype=bool)
        if _batch_ok(r, sigma, mask_b, groups):
            try:
                segs = [np.flatnonzero(g & mask_b) for g in groups]
                live = [k for k, idx in enumerate(segs) if idx.size >= 10]
                val = _search_segments(r, sigma, [segs[k] for k in live], _evaluator_for(evaluator, device))
                out = np.zeros_like(r)
                for v, k in zip(val, live):
                    if v is not None:
                        out[groups[k]] = v
                return out
            except _refused() as err:
                warnings.warn(f'calc_sigma_extra: {err}; using the host path')
                device = None
        else:
            warnings.warn('calc_sigma_extra: non-finite r or sigma (or sigma == 0) selected; using the per-group path')
    out = np.zeros_like(r)
    for group in sigma_extra_masks.values():
        sel = group & mask
        if np.sum(sel) < 10:
            continue
        rr, ss = r[sel], sigma[sel]
        if device is not None and np.all(np.isfinite(rr)) and np.all(np.isfinite(ss)):
            drde = DeviceRDE(rr, ss, device)
            cost = lambda s1: (drde(s1) - 1) ** 2  # noqa: E731
        else:
            drde = None
            cost = lambda s1: (RDE(rr / np.sqrt(s1 ** 2 + ss ** 2)) - 1) ** 2  # noqa: E731
        try:
            out[group] = scipyo.minimize_scalar(cost, method='bounded', bounds=[0, RDE(rr)])['x']
        except Exception as err:   # the reference prints and continues (calc_sigma_extra.py:42-43)
            print(err)
        finally:
            if drde is not None:
                drde.close()
    return out


def _on_grid_batched(x, y, r, sigma, in_TSE, groups, spacing, half, sigma_extra_max, make_eval):
    """calc_sigma_extra_on_grid with every (bin × group) search — and the all-points one per
    group — run together (_search_segments).  Bins are found per point, not per centre: a
    point's home centre is its rounded position, and the only centres within `half` of it are
    the home's lattice neighbours, so membership costs O(n) per neighbour offset.  Offsets are
    visited in ascending centre order, which keeps every point's weighted sums in the order the
    reference loop accumulates them (bit-identical result)."""
    n = r.size
    with np.errstate(invalid='ignore'):
        z = np.round((x + 1j * y) / spacing)
        centres, first, home = np.unique(z * spacing, return_index=True, return_inverse=True)
        kx, ky = np.real(z[first]).astype(np.int64), np.imag(z[first]).astype(np.int64)
    home = home.ravel()
    K = centres.size
    cre, cim = np.real(centres), np.imag(centres)
    m = int(np.floor(half / spacing + 0.5 + 1e-6))   # lattice reach of a bin from a point's home
    ky = ky - ky.min() + m
    NY = int(ky.max()) + m + 1
    key = kx * NY + ky
    order = np.argsort(key, kind='stable')
    key_sorted = key[order]
    # per neighbour offset (ascending centre order): the points inside that neighbour's bin
    member = []
    n_tse = np.zeros(K, dtype=np.int64)
    for di in range(-m, m + 1):
        for dj in range(-m, m + 1):
            tk = (kx + di) * NY + (ky + dj)
            pos = np.minimum(np.searchsorted(key_sorted, tk), K - 1)
            nbr = np.where(key_sorted[pos] == tk, order[pos], -1)
            cand = nbr[home]
            pts = np.flatnonzero(cand >= 0)
            c = cand[pts]
            dx, dy = np.abs(cre[c] - x[pts]), np.abs(cim[c] - y[pts])
            inside = (dx < half) & (dy < half)
            pts, c, dx, dy = pts[inside], c[inside], dx[inside], dy[inside]
            n_tse += np.bincount(c[in_TSE[pts]], minlength=K)
            member.append((pts, c, dx, dy))
    kept = n_tse >= 10      # a bin with fewer than 10 in-TSE points is dropped entirely
    member = [tuple(a[kept[c]] for a in (pts, c, dx, dy)) for pts, c, dx, dy in member]

    # segments: the all-points selection of every group, then (bin, group) in centre order
    segs, where = [], []    # where: (centre or -1, group)
    for g, group in enumerate(groups):
        idx = np.flatnonzero(group & in_TSE)
        if idx.size >= 10:
            segs.append(idx)
            where.append((-1, g))
    ctype = np.uint16 if K < 65536 else np.int64    # 16-bit keys: numpy's stable sort is a radix sort
    for g, group in enumerate(groups):
        P = np.concatenate([pts[in_TSE[pts] & group[pts]] for pts, c, _, _ in member])
        C = np.concatenate([c[in_TSE[pts] & group[pts]] for pts, c, _, _ in member])
        by_c = np.argsort(C.astype(ctype), kind='stable')
        P = P[by_c]
        cnt = np.bincount(C, minlength=K)
        start = np.concatenate([[0], np.cumsum(cnt)])
        for k in np.flatnonzero(cnt >= 10):   # a group with fewer than 10 selected points contributes 0
            segs.append(P[start[k]:start[k + 1]])
            where.append((int(k), g))
    val = _search_segments(r, sigma, segs, make_eval)

    full = np.zeros_like(r)
    V = np.zeros((K, len(groups)))
    ok = np.zeros((K, len(groups)), dtype=bool)
    for v, (k, g) in zip(val, where):
        if v is None:
            continue
        if k < 0:
            full[groups[g]] = v     # `where` lists the all-points segments in group order
        else:
            V[k, g], ok[k, g] = v, True
    wsum = np.zeros_like(r)
    wsig = np.zeros_like(r)
    for pts, c, dx, dy in member:
        s = np.zeros(pts.size)
        for g, group in enumerate(groups):   # later groups overwrite earlier ones, as out[group] = … does
            hit = group[pts] & ok[c, g]
            s[hit] = V[c[hit], g]
        if sigma_extra_max is not None:
            s = np.minimum(s, sigma_extra_max)
        W = (1 - dx / half) * (1 - dy / half)
        wsig[pts] += W * s
        wsum[pts] += W
    out = np.zeros_like(r) + full
    has = wsum > 0
    out[has] = wsig[has] / wsum[has]
    return out


def calc_sigma_extra_on_grid(x, y, r, sigma, in_TSE, sigma_extra_masks=None, spacing=1.e4, L_avg=None,
                             sigma_extra_max=None, device=None, evaluator=None):
    """Tent-weighted blend of sigma_extra estimated in overlapping square bins.  With `device`
    (GPU ordinal) every bin × group search runs in lock-step on the device's segmented select
    (_on_grid_batched; same result); `evaluator='host'` runs that batched path with np.sort."""
    L_avg = 2 * spacing if L_avg is None else L_avg
    if device is not None or evaluator is not None:
        masks = {'all': np.ones_like(r, dtype=bool)} if sigma_extra_masks is None else sigma_extra_masks
        groups = [np.asarray(g, dtype=bool) for g in masks.values()]
        tse = np.asarray(in_TSE, dtype=bool)
        if not (spacing > 0 and L_avg > 0):
            warnings.warn('calc_sigma_extra_on_grid: non-positive spacing; using the host path')
        elif not _batch_ok(r, sigma, tse, groups):
            warnings.warn('calc_sigma_extra_on_grid: non-finite r or sigma (or sigma == 0) selected; '
                          'using the host path')
        else:
            try:
                return _on_grid_batched(x, y, r, sigma, tse, groups, spacing, L_avg / 2, sigma_extra_max,
                                        _evaluator_for(evaluator, device))
            except _refused() as err:
                warnings.warn(f'calc_sigma_extra_on_grid: {err}; using the host path')
    full = calc_sigma_extra(r, sigma, in_TSE, sigma_extra_masks=sigma_extra_masks)
    centres = np.unique(np.round((x + 1j * y) / spacing) * spacing)
    wsum = np.zeros_like(r)
    wsig = np.zeros_like(r)
    half = L_avg / 2
    for c in centres:
        dx, dy = np.abs(np.real(c) - x), np.abs(np.imag(c) - y)
        inside = (dx < half) & (dy < half)
        sel = in_TSE & inside
        if np.sum(sel) < 10:
            continue
        s = calc_sigma_extra(r, sigma, sel, sigma_extra_masks=sigma_extra_masks)
        if sigma_extra_max is not None:
            s = np.minimum(s, sigma_extra_max)
        W = inside * (1 - dx / half) * (1 - dy / half)
        wsig += W * s
        wsum += W
    out = np.zeros_like(r) + full
    has = wsum > 0
    out[has] = wsig[has] / wsum[has]
    return out
