"""The segmented radix select of liblsqsurf (lsq_rde_create_segments / lsq_rde_select, rde.hip)
against np.sort, exactly: both paths (one workgroup with LDS-resident keys; multi-workgroup
histogram passes), the size thresholds between them, ties, the key range, the existing sort, the
argument checks, and calc_sigma_extra_on_grid / calc_sigma_extra end to end on the device."""
import ctypes
import importlib

import numpy as np
import pytest

from lssurf_amd._native import load, ptr
from lssurf_amd.calc_sigma_extra import calc_sigma_extra, calc_sigma_extra_on_grid
from test_sigma_extra_grid_host import grid_case

cse = importlib.import_module('lssurf_amd.calc_sigma_extra')

pytestmark = pytest.mark.gpu


def _ranks(n):
    _, j = cse._segment_ranks(n)
    return np.stack([j, j + 1], axis=1).ravel()


def _context(r, sigma, segs):
    seg_ptr = np.zeros(len(segs) + 1, dtype=np.int64)
    np.cumsum([s.size for s in segs], out=seg_ptr[1:])
    rank = np.stack([_ranks(s.size) for s in segs])
    return cse.DeviceSelect(r, sigma, seg_ptr, np.concatenate(segs), rank), rank


def _expected(r, sigma, segs, rank, active, s, raw):
    out = np.zeros((len(active), 4))
    for a, k in enumerate(active):
        rr, ss = r[segs[k]], sigma[segs[k]]
        with np.errstate(over='ignore'):    # the key-range case overflows to ±inf on purpose
            x = rr if raw else rr / np.sqrt(s[a] ** 2 + ss ** 2)
        out[a] = np.sort(x)[rank[k]]
    return out


@pytest.fixture(scope='module')
def sizes_case(gpu_available):
    small_max = int(load().lsq_rde_small_max())
    assert 1025 < small_max <= (160 * 1024) // 8
    sizes = [2, 3, 10, 63, 64, 65, 255, 256, 257, 1023, 1025, 2048, 2049, 8192, 8193,
             small_max - 1, small_max, small_max + 1, 100003]
    rng = np.random.default_rng(11)
    n = 120000
    r = 0.3 * rng.standard_t(3, n)
    sigma = rng.uniform(0.05, 0.2, n)
    segs = [rng.choice(n, m, replace=False).astype(np.int32) for m in sizes]   # overlapping index lists
    ctx, rank = _context(r, sigma, segs)
    yield dict(r=r, sigma=sigma, segs=segs, ctx=ctx, rank=rank, rng=rng)
    ctx.close()


@pytest.mark.parametrize('raw', [False, True])
def test_select_equals_sort_at_every_size(sizes_case, raw):
    c = sizes_case
    S = len(c['segs'])
    s = np.random.default_rng(5).uniform(0, 1.5, S)
    s[::4] = 0.0
    active = np.arange(S)
    got = c['ctx'](active, s, raw=raw)
    assert np.array_equal(got, _expected(c['r'], c['sigma'], c['segs'], c['rank'], active, s, raw))


def test_select_active_subset_in_shuffled_order(sizes_case):
    c = sizes_case
    S = len(c['segs'])
    active = np.random.default_rng(9).permutation(S)[:S // 2 + 1].astype(np.int32)
    s = np.linspace(0.0, 0.7, active.size)
    L = load()
    out = np.full((S, 4), -7.25)          # rows of inactive segments must stay as they are
    buf = np.zeros((active.size, 4))
    assert L.lsq_rde_select(c['ctx']._c, active.size, ptr(active), ptr(s), 0, ptr(buf)) == 0
    out[active] = buf
    want = _expected(c['r'], c['sigma'], c['segs'], c['rank'], active, s, False)
    assert np.array_equal(buf, want)
    assert np.array_equal(out[active], want)
    inactive = np.setdiff1d(np.arange(S), active)
    assert np.all(out[inactive] == -7.25)
    # the wrapper's own output has exactly one row per active segment
    assert c['ctx'](active, s).shape == (active.size, 4)


def _bit_mix(rng, m):
    """m finite doubles whose keys differ at every byte position: 64 random bit patterns, each
    repeated with its low 32, 16 and 8 bits re-drawn (and exact copies), plus the extremes."""
    base = rng.integers(0, 2 ** 63, 64, dtype=np.uint64) | (rng.integers(0, 2, 64, dtype=np.uint64) << np.uint64(63))
    bits = base[rng.integers(0, 64, m)]
    kind = rng.integers(0, 4, m)
    for k, nb in ((1, 32), (2, 16), (3, 8)):
        sel = kind == k
        mask = np.uint64((1 << nb) - 1)
        bits[sel] = (bits[sel] & ~mask) | (rng.integers(0, 2 ** 63, int(sel.sum()), dtype=np.uint64) & mask)
    v = bits.view(np.float64).copy()
    bad = ~np.isfinite(v)
    v[bad] = rng.standard_normal(int(bad.sum()))
    v[:10] = [1e300, -1e300, 1e-300, -1e-300, 0.0, -0.0, 1.5, -1.5, 5e-324, -5e-324]
    return v


@pytest.mark.parametrize('m', [1500, 40000])     # the LDS path and the multi-workgroup path
def test_select_ties_and_key_range(gpu_available, m):
    rng = np.random.default_rng(m)
    parts = {
        'rounded': np.round(0.3 * rng.standard_t(3, m), 1),       # heavy duplicates, v_j == v_{j+1}
        'equal': np.full(m, -0.625),
        'ascending': np.sort(rng.standard_normal(m)),
        'descending': np.sort(rng.standard_normal(m))[::-1],
        'mix': _bit_mix(rng, m),
        # ranks j_lo and j_lo+1 straddle the step: v_{j+1} is the smallest element above v_j
        'two_values': np.where(np.arange(m) <= _ranks(m)[0], -1.0, 2.0),
    }
    r = np.concatenate(list(parts.values()))
    sigma = np.full(r.size, 0.125)
    segs = [np.arange(k * m, (k + 1) * m, dtype=np.int32) for k in range(len(parts))]
    ctx, rank = _context(r, sigma, segs)
    try:
        active = np.arange(len(segs))
        for raw, s in ((True, np.zeros(len(segs))), (False, np.full(len(segs), 0.25)), (False, np.zeros(len(segs)))):
            got = ctx(active, s, raw=raw)
            want = _expected(r, sigma, segs, rank, active, s, raw)
            assert np.all(got == want), (raw, s[0], got, want)     # ±0 may differ in sign
        v = ctx(active, np.zeros(len(segs)), raw=True)
        assert v[1, 0] == v[1, 1] == v[1, 3] == -0.625
        assert (v[5, 0], v[5, 1]) == (-1.0, 2.0)
    finally:
        ctx.close()


def test_select_equals_existing_sort(sizes_case):
    """One 100 003-point segment: lsq_rde_select against lsq_rde_order_stats (hipcub radix sort)."""
    c = sizes_case
    k = len(c['segs']) - 1
    idx = c['segs'][k]
    assert idx.size == 100003
    rr, ss = np.ascontiguousarray(c['r'][idx]), np.ascontiguousarray(c['sigma'][idx])
    L = load()
    old = L.lsq_rde_create(0, rr.size, ptr(rr), ptr(ss))
    assert old
    try:
        ranks = np.ascontiguousarray(c['rank'][k], dtype=np.int64)
        for s in (0.0, 0.21, 3.0):
            v = np.zeros(4)
            assert L.lsq_rde_order_stats(old, s, 4, ptr(ranks), ptr(v)) == 0
            assert np.array_equal(c['ctx'](np.array([k]), np.array([s]))[0], v)
        # each kind of context refuses the other's call
        seg, sv, out = np.zeros(1, np.int32), np.zeros(1), np.zeros(4)
        assert L.lsq_rde_select(old, 1, ptr(seg), ptr(sv), 0, ptr(out)) == -2
        assert L.lsq_rde_last_error(old)
        assert L.lsq_rde_order_stats(c['ctx']._c, 0.1, 4, ptr(ranks), ptr(out)) == -2
        assert L.lsq_rde_last_error(c['ctx']._c)
    finally:
        L.lsq_rde_destroy(old)


def test_select_argument_errors(sizes_case):
    L = load()
    r, sigma = np.arange(20.), np.ones(20)
    idx = np.arange(20, dtype=np.int32)

    def create(seg_ptr, seg_idx, rank):
        seg_ptr, rank = np.asarray(seg_ptr, np.int64), np.asarray(rank, np.int64)
        status = ctypes.c_int(99)
        c = L.lsq_rde_create_segments(0, 20, ptr(r), ptr(sigma), seg_ptr.size - 1, ptr(seg_ptr), ptr(seg_idx),
                                      ptr(rank), ctypes.byref(status))
        return c, status.value, L.lsq_rde_last_error(None).decode()

    good, st, _ = create([0, 10, 20], idx, [1, 2, 7, 8, 1, 2, 7, 8])
    assert good and st == 0
    L.lsq_rde_destroy(good)
    bad_idx = idx.copy()
    bad_idx[13] = 20
    for seg_ptr, seg_idx, rank in (([0, 10, 20], idx, [1, 2, 7, 8, 1, 2, 9, 10]),      # rank >= segment size
                                   ([0, 12, 10, 20], idx, [1, 2, 7, 8] * 3),           # non-monotone seg_ptr
                                   ([0, 10, 20], bad_idx, [1, 2, 7, 8, 1, 2, 7, 8])):  # index >= n
        c, st, msg = create(seg_ptr, seg_idx, rank)
        assert not c and st == -2 and msg
    ctx = sizes_case['ctx']
    out = np.zeros(4)
    for seg in (len(sizes_case['segs']), -1):                                          # segment id out of range
        seg = np.array([seg], np.int32)
        assert L.lsq_rde_select(ctx._c, 1, ptr(seg), ptr(np.zeros(1)), 0, ptr(out)) == -2
        assert L.lsq_rde_last_error(ctx._c)


def test_on_grid_device_equals_host(gpu_available):
    case = grid_case()
    assert np.array_equal(calc_sigma_extra_on_grid(**case, device=0), calc_sigma_extra_on_grid(**case))


def test_two_groups_device_equals_host(gpu_available):
    case = grid_case()
    args = (case['r'], case['sigma'], case['in_TSE'], case['sigma_extra_masks'])
    assert np.array_equal(calc_sigma_extra(*args, device=0), calc_sigma_extra(*args))
