#!/usr/bin/env python3
"""Host check of the lumped extra rows' tables (csrc/xr_lump.hpp), without a GPU.

Builds tools/xr_lump_check.cpp (with --sanitize: -fsanitize=address,undefined), feeds it the row
sets of tests/test_gpu_mg_priors.py on t64 and t15 as the device keeps them (duplicates merged,
zeros and removed columns dropped), and compares the level-1 blocks that k_mg_lump_xr would sum from
the tables, B_1[m] = Σ_r rs_r² w¹_{m,r} τ τᵀ, with tests/mg_host.py's lumping of Pᵀ XᵀW²X P.
Also feeds rows over non-adjacent epochs and expects the refusal.

Usage: python tools/xr_lump_check.py [--sanitize]
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def build(sanitize, out):
    cxx = shutil.which('g++') or shutil.which('c++') or '/opt/rocm/llvm/bin/clang++'
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-Wall', os.path.join(ROOT, 'tools', 'xr_lump_check.cpp'), '-o', out]
    if sanitize:
        cmd[1:1] = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    subprocess.run(cmd, check=True)


def formed(csr, keep_cols, n_full):
    """the rows as the device keeps them: CSR over the full ids, columns ascending"""
    X = sp.csr_matrix((csr[2].copy(), csr[1].copy(), csr[0].copy()), shape=(csr[0].size - 1, n_full))
    X.sum_duplicates()
    X.eliminate_zeros()
    kept = np.zeros(n_full)
    kept[keep_cols] = 1.
    X = (X @ sp.diags(kept)).tocsr()
    X.eliminate_zeros()
    X.sort_indices()
    return X


def tables(exe, geom, X, long_rows=64):
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, 'in'), os.path.join(d, 'out')
        with open(fin, 'wb') as f:
            np.array(list(geom) + [long_rows, X.shape[0], X.nnz], np.int64).tofile(f)
            X.indptr.astype(np.int64).tofile(f)
            X.indices.astype(np.int64).tofile(f)
            X.data.astype(np.float64).tofile(f)
        subprocess.run([exe, fin, fout], check=True)
        raw = open(fout, 'rb').read()
    head = np.frombuffer(raw, np.int64, 5)
    if not head[0]:
        return {'ok': False, 'why': raw[40:].decode()}
    m_x, nn, ne, nl = X.shape[0], int(head[2]), int(head[3]), int(head[4])
    o = 40
    out = {'ok': True, 'rows': int(head[1])}
    for name, dt, n in (('tau', np.float64, 4 * m_x), ('node', np.int32, nn), ('ptr', np.int64, nn + 1),
                        ('row', np.int32, ne), ('w', np.float64, ne), ('long', np.int32, nl)):
        out[name] = np.frombuffer(raw, dt, n, o)
        o += n * np.dtype(dt).itemsize
    assert o == len(raw)
    return out


def lumped_matrix(T, rs, nyc, nxc, nt):
    """the level-1 operator of the blocks the kernels sum: full space [z0 (nodes); dz (nodes · nt)]"""
    nodes = nyc * nxc
    tau = T['tau'].reshape(-1, 4)
    r, c, v = [], [], []
    for j, m in enumerate(T['node']):
        for k in range(T['ptr'][j], T['ptr'][j + 1]):
            row = T['row'][k]
            cc = rs[row] ** 2 * T['w'][k]
            tz, ta, tb, t = tau[row]
            t = int(t)
            z, a = m, nodes + m * nt + t
            ent = [(z, z, tz * tz), (z, a, tz * ta), (a, z, tz * ta), (a, a, ta * ta)]
            if t + 1 < nt:
                b = a + 1
                ent += [(z, b, tz * tb), (b, z, tz * tb), (b, b, tb * tb), (a, b, ta * tb), (b, a, ta * tb)]
            for i, jj, x in ent:
                r.append(i), c.append(jj), v.append(cc * x)
    n = nodes * (1 + nt)
    return sp.csr_matrix((v, (r, c)), shape=(n, n))


def main():
    sanitize = '--sanitize' in sys.argv
    import test_gpu_mg_priors as T
    from mg_host import lump_by_node, node_of, prolong_full, slot_of
    from test_gpu_priors import _csr
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, 'xr_lump_check')
        build(sanitize, exe)
        for name in ('t64', 't15'):
            S, kw, keep_cols = T._host_of(name)
            ny, nx, nt = S['grids']['dz'].shape
            n_full = S['Gc'].col_N
            assert S['grids']['z0'].col_0 == 0 and S['grids']['dz'].col_0 == ny * nx
            geom = (ny, nx, nt, 1, 0, ny * nx, ny // 2 + 1, nx // 2 + 1)
            for label, csr in (('frame', T._rows_frame(name)), ('interp', T._rows_interp(name)),
                               ('edge', T._rows_edge(name)), ('all', T._rows_all(name))):
                X = formed(csr, keep_cols, n_full)
                wx, kx = T._weights(X.shape[0], 43)
                rs = wx * kx
                tab = tables(exe, geom, X)
                assert tab['ok'], tab
                assert np.all(np.diff(tab['node']) > 0)
                for j in range(tab['node'].size):
                    assert np.all(np.diff(tab['row'][tab['ptr'][j]:tab['ptr'][j + 1]]) > 0)   # rows ascend
                got = lumped_matrix(tab, rs, geom[6], geom[7], nt)
                Xw = sp.diags(rs) @ X
                P, nyc, nxc = prolong_full(ny, nx, nt)
                ref = lump_by_node((P.T @ (Xw.T @ Xw) @ P).tocsr(), node_of(nyc, nxc, nt), slot_of(nyc, nxc, nt))
                err = abs(got - ref).max() / abs(ref).max()
                print(f'{name} {label}: rows {X.shape[0]} ({tab["rows"]} with entries), nodes {tab["node"].size} '
                      f'({tab["long"].size} long), entries {tab["row"].size}, err {err:.2e}')
                assert err <= 1e-13, err
            # non-adjacent epochs: refused, the first such row named
            col = lambda t: ny * nx + (3 * nx + 4) * nt + t   # noqa: E731
            ref_t = kw['reference_epoch']
            t0 = next(t for t in range(nt - 3) if ref_t not in (t, t + 1, t + 3))
            bad = formed(_csr([([col(t0), col(t0 + 1)], [1., 1.]), ([col(t0), col(t0 + 3)], [1., -1.])]),
                         keep_cols, n_full)
            tab = tables(exe, geom, bad)
            print(name, 'refusal:', tab)
            assert not tab['ok'] and 'extra row 1 ' in tab['why']
    print('xr_lump_check: ok' + (' (address + undefined behaviour sanitizers)' if sanitize else ''))


if __name__ == '__main__':
    main()
