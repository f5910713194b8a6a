"""Design experiment (CPU, scipy) behind lsq_set_extra_rows_lumping: PCG iteration counts on the
smooth_fit normal equations with dz priors, for the multigrid V-cycle of tools/mg_proto.py with the
priors' rows carried in three ways.  Not product code.

System: t64 (64 × 64 × 12, 8 192 points) with the tile-edge frame of tools/prior_step.py::frame_rows
scaled to it (a 49-node tile with 2-node strips, every non-reference epoch: 4 136 rows of 1 at the
node and −1 at its reference-epoch column), weights 1/σ, priors N(0, 0.05).  PCG to a 1e-10
relative residual.  Level 0 (operator, node blocks, λ) is exact in the first three variants:

  lumped      the weighted prior rows stacked behind the data rows, so build_levels(lump=True) lumps
              them per coarse node exactly as it lumps data rows — what the device does
  level0      level 0 from the system with priors, the coarse levels from the system without
  none        the whole hierarchy from the system without priors

usage: python tools/mg_prior_proto.py [t64] [sigma ...]      (default σ: 0.1 0.01)
"""
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, __file__.rsplit('/tools/', 1)[0] + '/tools')
from mg_proto import BJ, blocks_of, build_levels, pcg, system, vcycle  # noqa: E402
from prior_step import frame_rows  # noqa: E402
from lssurf_amd import synthetic  # noqa: E402

TOL = 1e-10


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else 't64'
    sigmas = [float(s) for s in sys.argv[2:]] or [0.1, 0.01]
    A, b, keep, grids, n_data = system(cfg)
    gd = grids['dz']
    ny, nx, nt = gd.shape
    ref = synthetic.points(cfg)[1]['reference_epoch']
    tile = 49 if cfg == 't64' else int(round(0.77 * min(ny, nx)))
    ip, cols, vals = frame_rows(gd, ref, tile, 2)
    m_x = ip.size - 1
    n_full = ny * nx * (1 + nt)
    X = sp.csr_matrix((vals, cols, ip), shape=(m_x, n_full))[:, keep].tocsr()
    prior = 0.05 * np.random.default_rng(1).standard_normal(m_x)
    ptr, bcols = blocks_of(ny, nx, nt, keep)
    mg = lambda levels: (lambda r: vcycle(levels, 0, r))   # noqa: E731
    print(f'{cfg}: {A.shape[0]} rows, {A.shape[1]} columns, {m_x} prior rows, tol {TOL}', flush=True)

    N0 = (A.T @ A).tocsr()
    plain = build_levels(A, keep, grids, deg=2, lump=True, n_data=n_data)
    _, it_bj0 = pcg(N0, A.T @ b, BJ(N0, ptr, bcols), TOL)
    _, it_mg0 = pcg(N0, A.T @ b, mg(plain), TOL)
    print(f'no priors: block-Jacobi {it_bj0}, multigrid {it_mg0}', flush=True)
    for sigma in sigmas:
        t0 = time.time()
        Xw = (X / sigma).tocsr()
        A2 = sp.vstack([A[:n_data], Xw, A[n_data:]]).tocsr()
        b2 = np.r_[b[:n_data], prior / sigma, b[n_data:]]
        N, rhs = (A2.T @ A2).tocsr(), A2.T @ b2
        x_bj, it_bj = pcg(N, rhs, BJ(N, ptr, bcols), TOL, maxit=20000)
        lumped = build_levels(A2, keep, grids, deg=2, lump=True, n_data=n_data + m_x)
        x_l, it_l = pcg(N, rhs, mg(lumped), TOL, maxit=20000)
        _, it_0 = pcg(N, rhs, mg([lumped[0]] + plain[1:]), TOL, maxit=20000)
        _, it_n = pcg(N, rhs, mg(plain), TOL, maxit=20000)
        rel = np.linalg.norm(x_l - x_bj) / np.linalg.norm(x_bj)
        print(f'sigma {sigma}: block-Jacobi {it_bj}; multigrid lumped {it_l} (rel diff to block-Jacobi {rel:.1e}), '
              f'level0 {it_0}, none {it_n}  ({time.time() - t0:.0f} s)', flush=True)


if __name__ == '__main__':
    main()
