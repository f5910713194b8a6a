#!/usr/bin/env python3
"""Binned sigma_extra at C4 size: calc_sigma_extra_on_grid on the host loop (the path before the
segmented select existed) against the device path, and one lsq_rde_select evaluation over every
segment against one lsq_rde_order_stats sort of all points.

Input: the 2 M points of synthetic.points('c4'), residuals of one smooth_fit solve
(max_iterations=1), 10 km bins, one group, every point in in_TSE.  Every timed call ends in a
device synchronise (the library calls return after their stream has drained), so the figures are
host wall clock around synchronous calls; the device path is warmed up once first.

Usage: python tools/sebin_c4.py OUT.json [--config c4] [--spacing 1e4] [--reps 5] [--no-host]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('--config', default='c4')
    ap.add_argument('--spacing', type=float, default=1e4)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-host', action='store_true', help='skip the (slow) host loop')
    a = ap.parse_args()

    import lssurf_amd as LS
    from lssurf_amd import synthetic
    from lssurf_amd._native import load, ptr
    cse = importlib.import_module('lssurf_amd.calc_sigma_extra')

    D, kw = synthetic.points(a.config)
    S = LS.smooth_fit(data=D, VERBOSE=False, max_iterations=1, **kw)
    d = S['data']
    x, y, sigma = np.asarray(d.x), np.asarray(d.y), np.asarray(d.sigma)
    r = np.asarray(d.z) - np.asarray(d.z_est)
    in_TSE = np.ones(r.size, dtype=bool)
    res = {'config': a.config, 'n_points': int(r.size), 'spacing': a.spacing,
           'n_centres': int(np.unique(np.round((x + 1j * y) / a.spacing) * a.spacing).size)}

    def on_grid(**k):
        return cse.calc_sigma_extra_on_grid(x, y, r, sigma, in_TSE, spacing=a.spacing, **k)

    # the evaluator calls of one device run: segments, evaluations, time inside the evaluator
    stats = {'calls': 0, 'segments': 0, 'active': 0, 'entries': 0, 'eval_s': 0.0, 'create_s': 0.0}

    class Timed(cse.DeviceSelect):
        def __init__(self, *args):
            t = time.perf_counter()
            super().__init__(*args, device=0)
            stats['create_s'] += time.perf_counter() - t
            stats['segments'] = int(self.ptr.size - 1)
            stats['entries'] = int(self.ptr[-1])

        def __call__(self, seg, s, raw=False):
            t = time.perf_counter()
            out = super().__call__(seg, s, raw)
            stats['eval_s'] += time.perf_counter() - t
            stats['calls'] += 1
            stats['active'] += len(seg)
            return out

    on_grid(device=0)                                   # warm-up: code objects, allocator
    walls = []
    for _ in range(a.reps):
        for k in stats:
            stats[k] = 0
        t = time.perf_counter()
        dev = on_grid(evaluator=Timed)
        walls.append(time.perf_counter() - t)
    res['device_wall_s'] = float(np.median(walls))
    res['device_wall_all_s'] = walls
    res['device_breakdown_last'] = dict(stats)

    if not a.no_host:
        t = time.perf_counter()
        host = on_grid()
        res['host_wall_s'] = time.perf_counter() - t
        res['device_equals_host'] = bool(np.array_equal(dev, host))

    # one select evaluation over all segments vs one sort of all points
    centres_all = [np.arange(r.size)]
    seg_ptr = np.array([0, r.size], dtype=np.int64)
    L = load()
    # (a) every segment of the binned call, one lsq_rde_select
    captured = {}

    class Capture(cse.DeviceSelect):
        def __init__(self, *args):
            super().__init__(*args, device=0)
            captured['ev'] = self

        def close(self):     # keep the context for the timing below
            pass

    on_grid(evaluator=Capture)
    ev = captured['ev']
    n_seg = ev.ptr.size - 1
    seg, s = np.arange(n_seg, dtype=np.int32), np.full(n_seg, 0.05)
    ev(seg, s)
    ts = []
    for _ in range(max(a.reps, 10)):
        t = time.perf_counter()
        ev(seg, s)
        ts.append(time.perf_counter() - t)
    cse.DeviceSelect.close(ev)
    res['select_all_segments_s'] = float(np.median(ts))
    res['select_segments'] = int(n_seg)
    res['select_entries'] = int(ev.ptr[-1])
    # (b) the all-points segment alone, select vs the existing sort
    rank = np.stack([cse._segment_ranks(r.size)[1] + k for k in (0, 1)], axis=1).ravel()[None, :]
    one = cse.DeviceSelect(r, sigma, seg_ptr, centres_all[0].astype(np.int32), rank)
    one(np.zeros(1, np.int32), np.array([0.05]))
    ts = []
    for _ in range(max(a.reps, 10)):
        t = time.perf_counter()
        v_sel = one(np.zeros(1, np.int32), np.array([0.05]))
        ts.append(time.perf_counter() - t)
    one.close()
    res['select_all_points_s'] = float(np.median(ts))
    old = L.lsq_rde_create(0, r.size, ptr(r), ptr(sigma))
    idx, v = np.ascontiguousarray(rank[0], dtype=np.int64), np.zeros(4)
    L.lsq_rde_order_stats(old, 0.05, 4, ptr(idx), ptr(v))
    ts = []
    for _ in range(max(a.reps, 10)):
        t = time.perf_counter()
        L.lsq_rde_order_stats(old, 0.05, 4, ptr(idx), ptr(v))
        ts.append(time.perf_counter() - t)
    L.lsq_rde_destroy(old)
    res['sort_all_points_s'] = float(np.median(ts))
    res['select_equals_sort'] = bool(np.array_equal(v_sel[0], v))
    res['timing'] = 'host wall clock around synchronous library calls, medians'

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
