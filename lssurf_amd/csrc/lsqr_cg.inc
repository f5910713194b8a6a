// lsqr_cg.inc — CGNR (lsq_opts.method = 1): preconditioned conjugate gradients on the normal
// equations AᵀA x = Aᵀb of a structured stencil system (BASELINE.json north star: "CGNR/LSQR").
// Included by lsqr.hip in namespace lsq.
//
// Why: at C4, 73 M of the 75 M rows are stencil rows.  LSQR must stream its m-vector u over
// them twice per iteration (24 B/row); CG on AᵀA works in the column space only.  AᵀA of the
// stencil rows is applied as a NORMAL STENCIL: for a grid and its parts (constant row scale w_q),
//   (AᵀA)_{c, c+d} = Σ_q w_q² Σ_{t1,t2: o_t2 − o_t1 = d} v_t1 v_t2 · [c − o_t1 ∈ box_q]
// depends on c only through its boundary class per dim (system.hpp CgGrid), so one coefficient
// row per class (a few hundred classes × ≤ 64 offsets, L2 resident) replaces 73 M rows.  The data
// rows (bi/trilinear interpolation) are applied as Adᵀ(Ad p): without a stored matrix from the
// points' float subscripts sorted by cell (k_cg_dmf_*, DmfDesc) when the interpolation grids share
// one (y, x) lattice, else through the SELL Ad / CSR ATd copies (k_cg_data, k_cg_atdq).
//
// One iteration = five launches, scalars on the device:
//   k_cg_data    t = Ad·p,  p = z + β p_old gathered on the fly           (data rows)
//   k_cg_normal  p = z + β p_old staged per tile in LDS (written once), q = N p + ATd·t, Σ p·q
//                (k_cg_normal_chunk where a tile of whole dim-2 columns exceeds LDS: lsq_set_cg_chunks)
//                (lsq_set_cg_tile_dmf: the <false> instantiations, q = N_s p alone, then column mode's
//                matrix-free k_cg_dmf_ad, the eliminations and k_cg_dmf_atq / k_cg_dmf_atq_long)
//   k_cg_alpha   α = ρ / pᵀq; Lanczos-derived ‖A‖ and ‖Δx‖ estimates               (1 block)
//   k_cg_block   x += α p, s −= α q, z = M⁻¹ s (block-Jacobi R_b⁻¹R_b⁻ᵀ, or Jacobi), Σ sᵀz
//   k_cg_beta    β = ρ'/ρ, ‖r‖² −= α ρ, LSQR stopping rules                         (1 block)
// Preconditioners: M = blockdiag(R_bᵀR_b) = the (y, x)-node blocks of AᵀA (precond 3), or
// diag(AᵀA) (precond 1).  In exact arithmetic the iterates equal LSQR's on A·M^{-1/2} (same
// Krylov space, same minimised residual), so "iterations" count the same unit of progress.
//
// Where to add a term to the operator: cg_launch_apply (q = N p, the stages of enum CgStage) and
// cg_launch_update (α, update, β) spell the plain step once.  The profilers (cg_profile_steps), the
// test hook cg_apply_normal and the ranks of a group (group_cg_iteration) all run it; only
// cg_launch_iteration's two tuned column-mode branches spell their own overlapped order from the
// same helpers.  The multigrid's level-0 operator (mg.inc, mg_launch_op) carries no elimination on
// purpose and is separate.

namespace {

__device__ __forceinline__ int cg_cls(int c, int n, int K, int ncls) {
    return ncls == n ? c : (c < K ? c : (c >= n - K ? c - n + 2 * K + 1 : K));
}

// Σ_k val·(z + β p_old)[col] over a SELL-64 row (the data rows of Ad)
__device__ __forceinline__ double sell_row_dot_zp(const int32_t* __restrict__ ci, const double* __restrict__ val,
                                                  int64_t base, int64_t W, int lane, const double* __restrict__ z,
                                                  const double* __restrict__ p, double beta) {
    const int32_t* c = ci + base + lane;
    const double* v = val + base + lane;
    double a0 = 0.0, a1 = 0.0;
    int64_t k = 0;
    for (; k + 2 <= W; k += 2) {
        const int32_t c0 = c[(k + 0) * SELL_C], c1 = c[(k + 1) * SELL_C];
        const double v0 = v[(k + 0) * SELL_C], v1 = v[(k + 1) * SELL_C];
        a0 += v0 * (z[c0] + beta * p[c0]);
        a1 += v1 * (z[c1] + beta * p[c1]);
    }
    for (; k < W; ++k) {
        const int32_t c0 = c[k * SELL_C];
        a0 += v[k * SELL_C] * (z[c0] + beta * p[c0]);
    }
    return a0 + a1;
}

__global__ __launch_bounds__(BLOCK) void k_cg_data(const CgState* __restrict__ st, int64_t npts, int64_t nslices,
                                                   const int64_t* __restrict__ sp, const int32_t* __restrict__ ci,
                                                   const double* __restrict__ val, const double* __restrict__ z,
                                                   const double* __restrict__ pold, double* __restrict__ td,
                                                   double* __restrict__ part) {
    if (st->stop) return;
    const double beta = st->beta;
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double tt = 0.0;   // ‖Ad p‖² = pᵀAdᵀ(Ad p): the data rows' share of pᵀq (column mode)
    for (int64_t s = (int64_t)blockIdx.x * 4 + wid; s < nslices; s += (int64_t)gridDim.x * 4) {
        const int64_t row = s * SELL_C + lane;
        if (row < npts) {
            const int64_t base = sp[s];
            const int64_t W = (sp[s + 1] - base) / SELL_C;
            const double t = pold ? sell_row_dot_zp(ci, val, base, W, lane, z, pold, beta) : sell_row_dot(ci, val, base, W, lane, z);
            td[row] = t;
            tt += t * t;
        }
    }
    if (part) store_partial(tt, part, blockIdx.x);
}

// tile id of this workgroup: consecutive tiles stay on one XCD (workgroups are dealt to the 8
// XCDs round robin), so a tile's y-halo rows are in the L2 its neighbours just filled.  The
// grid is launched with 8·ceil(T/8) workgroups; ids ≥ T idle.
__device__ __forceinline__ int cg_tile_of_block() {
    const int per = (int)(gridDim.x >> 3);
    return (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
}
// the same for workgroup b of n (n a multiple of 8): XCD b mod 8 gets the contiguous ids
// [(b mod 8)·n/8, (b mod 8 + 1)·n/8) — the data kernels' neighbouring points / strips share
// their p and q lines in that XCD's L2 instead of being fetched by all eight
__device__ __forceinline__ int xcd_block(int b, int n) { return (b & 7) * (n >> 3) + (b >> 3); }

// Stage p = z + β p_old over a tile (rows y0 − hy .. y0 + ty + hy − 1, dim-1 positions
// x0 − hx .. x0 + CG_TX + hx − 1, all of dim 2) into L: image index front + (r·wx + xi)·tpad + t,
// zeros outside the grid, in the dim-2 padding and in the front/back pads.  The tile's own nodes
// are written back as the new p.  CG_SU elements in flight per thread.
constexpr int CG_SU = 6;
__device__ __forceinline__ void cg_stage_p(const CgGrid& C, int y0, int x0, double beta, const double* __restrict__ z,
                                           const double* __restrict__ pold, double* __restrict__ pnew, double* L) {
    const int S0 = C.shape[0], S1 = C.shape[1], S2 = C.shape[2];
    const int hy = C.hy, hx = C.hx, tpad = C.tpad, front = C.front;
    const int rowlen = C.wx * tpad, img = (C.ty + 2 * hy) * rowlen, lds = C.lds;
    const int64_t col0 = C.col0;
    for (int i0 = threadIdx.x; i0 < lds; i0 += CG_SU * BLOCK) {
        int64_t gi[CG_SU];
        bool ld[CG_SU], own[CG_SU];
#pragma unroll
        for (int k = 0; k < CG_SU; ++k) {
            const int i = i0 + k * BLOCK, ii = i - front;
            ld[k] = own[k] = false;
            gi[k] = 0;
            if (i < lds && ii >= 0 && ii < img) {
                const int r = (int)fdiv((uint32_t)ii, C.fd_row);
                const int rem = ii - r * rowlen;
                const int xi = (int)fdiv((uint32_t)rem, C.fd_pad);
                const int t = rem - xi * tpad;
                const int y = y0 - hy + r, x = x0 - hx + xi;
                if (t < S2 && y >= 0 && y < S0 && x >= 0 && x < S1) {
                    ld[k] = true;
                    gi[k] = col0 + ((int64_t)y * S1 + x) * S2 + t;
                    own[k] = r >= hy && r < hy + C.ty && xi >= hx && xi < hx + CG_TX;
                }
            }
        }
        double zv[CG_SU], pv[CG_SU];
#pragma unroll
        for (int k = 0; k < CG_SU; ++k) {
            zv[k] = ld[k] && z ? z[gi[k]] : 0.0;
            pv[k] = ld[k] && z ? pold[gi[k]] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < CG_SU; ++k) {
            const int i = i0 + k * BLOCK;
            if (i < lds) {
                const double v = zv[k] + beta * pv[k];
                L[i] = v;
                if (own[k]) pnew[gi[k]] = v;
            }
        }
    }
}

// Column mode, one iteration: q += ATd·t in node-enumeration order.  A wave takes 256
// consecutive rows (4 per lane, lane-contiguous); the row ends come from the next lane, the first
// two entries of every row and the q values are in flight together (dz rows hold 1–2 entries),
// longer rows (z0: ~8) finish in csr_row_dot.
constexpr int CG_AR = 4;
__global__ __launch_bounds__(BLOCK) void k_cg_atdq(const CgState* __restrict__ st, const MfDesc* __restrict__ md,
                                                   const int32_t* __restrict__ arp, const int32_t* __restrict__ aci,
                                                   const double* __restrict__ aval, const double* __restrict__ td,
                                                   double* __restrict__ q) {
    if (st->stop) return;
    const int lane = threadIdx.x & 63;
    const int64_t nodes = md->nodes;
    const int64_t base = ((int64_t)blockIdx.x * BLOCK + (threadIdx.x & ~63)) * CG_AR;
    int a[CG_AR], b[CG_AR];
    int64_t col[CG_AR];
    double qv[CG_AR];
#pragma unroll
    for (int k = 0; k < CG_AR; ++k) {
        const int64_t pos = base + 64 * k + lane;
        a[k] = pos < nodes ? arp[pos] : 0;
        b[k] = __shfl_down(a[k], 1, 64);
        if (lane == 63 && pos < nodes) b[k] = arp[pos + 1];
        col[k] = -1;
        for (int g = 0; g < md->n_grids; ++g) {
            const MfGrid& G = md->g[g];
            if (G.nparts && pos >= G.node0 && pos < (int64_t)G.node0 + G.nodes) col[k] = G.col0 + (pos - G.node0);
        }
        if (pos >= nodes || b[k] == a[k]) col[k] = -1;
        qv[k] = col[k] >= 0 ? q[col[k]] : 0.0;
    }
    int c0[CG_AR], c1[CG_AR];
    double v0[CG_AR], v1[CG_AR];
#pragma unroll
    for (int k = 0; k < CG_AR; ++k) {
        const int n = b[k] - a[k];
        const int i0 = n > 0 ? a[k] : 0, i1 = n > 1 ? a[k] + 1 : 0;
        c0[k] = aci[i0];
        c1[k] = aci[i1];
        v0[k] = n > 0 ? aval[i0] : 0.0;
        v1[k] = n > 1 ? aval[i1] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < CG_AR; ++k) {
        double acc = v0[k] * td[c0[k]] + v1[k] * td[c1[k]];
        if (b[k] - a[k] > 2) acc += csr_row_dot(aci, aval, a[k] + 2, b[k], td);
        if (col[k] >= 0) q[col[k]] = qv[k] + acc;
    }
}

// ---- matrix-free data rows (DmfDesc) ----------------------------------------------------------
#ifndef DMF_U_DEF
#define DMF_U_DEF 4
#endif
constexpr int DMF_U = DMF_U_DEF;   // k_cg_dmf_atq: points in flight per thread
// cell of a float subscript and the fraction within it, clamped to the last cell (f = S−1 exactly:
// cell S−2, fraction 1 — the same weights on the same nodes as k_gen_rows' cell S−1, fraction 0)
__device__ __forceinline__ int dmf_cell(double f, int S, double& fr) {
    const double cf = floor(f);
    int c = (int)cf;
    fr = f - cf;
    if (c > S - 2 || c < 0) {
        c = c < 0 ? 0 : S - 2;
        fr = f - (double)c;
    }
    return c;
}

// t = Ad·p, one thread per sorted point: the 4 (2-D) and 8 (3-D) interpolation weights of
// lin_op.interp_mtx (w = ((1·a_y)·a_x)·a_t) from the point's float subscripts, p gathered at the
// cell's corners; td = rs·t (the row scale AdᵀAd needs twice), partial ‖t‖².
// (bid, nblk: the workgroup's index among the nblk that share the points)
// (points in one contiguous chunk per workgroup, chunks XCD-contiguous: xcd_block; nblk % 8 == 0)
#ifndef DMF_AD_U
#define DMF_AD_U 2
#endif
// DMF_AD_U points per thread and trip (their P loads, then their gathers, issued together; the
// partial Σt² still adds the points in the one-per-trip order)
__device__ __forceinline__ void cg_dmf_ad_body(const DmfDesc& D, const double4* __restrict__ pt,
                                               const double* __restrict__ p, double* __restrict__ td,
                                               double* __restrict__ part, int bid, int nblk) {
    constexpr int U = DMF_AD_U;
    double tt = 0.0;
    const int64_t S1 = D.S1, S2 = D.S2;
    const int64_t chunk = (D.npts + (int64_t)nblk * BLOCK - 1) / ((int64_t)nblk * BLOCK) * BLOCK;
    const int64_t i0 = (int64_t)xcd_block(bid, nblk) * chunk, i1 = min(i0 + chunk, D.npts);
    for (int64_t ib = i0 + threadIdx.x; ib < i1; ib += U * BLOCK) {
        double4 P[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = ib + u * BLOCK;
            P[u] = i < i1 ? pt[i] : make_double4(0.0, 0.0, 0.0, 0.0);
        }
        double acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double fy, fx;
            const int cy = dmf_cell(P[u].x, D.S0, fy), cx = dmf_cell(P[u].y, D.S1, fx);
            const double ay = 1.0 - fy, ax = 1.0 - fx;
            const double w00 = ay * ax, w01 = ay * fx, w10 = fy * ax, w11 = fy * fx;
            const int64_t nd = (int64_t)cy * S1 + cx;
            double a = 0.0;
            for (int k = 0; k < D.n2; ++k) {
                const double* __restrict__ q = p + D.col2[k] + nd;
                a += w00 * q[0] + w01 * q[1] + w10 * q[S1] + w11 * q[S1 + 1];
            }
            if (D.n3) {
                double ft;
                const int ct = dmf_cell(P[u].z, D.S2, ft);
                const double at = 1.0 - ft;
                const double* __restrict__ q = p + D.col3 + nd * S2 + ct;
                const int64_t X = S2, Y = S1 * S2;
                a += (w00 * at) * q[0] + (w00 * ft) * q[1] + (w01 * at) * q[X] + (w01 * ft) * q[X + 1] +
                     (w10 * at) * q[Y] + (w10 * ft) * q[Y + 1] + (w11 * at) * q[Y + X] + (w11 * ft) * q[Y + X + 1];
            }
            acc[u] = a;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = ib + u * BLOCK;
            if (i < i1) {
                const double t = P[u].w * acc[u];
                td[i] = P[u].w * t;
                tt += t * t;
            }
        }
    }
    store_partial(tt, part, bid);
}

__global__ __launch_bounds__(BLOCK) void k_cg_dmf_ad(const CgState* __restrict__ st, DmfDesc D,
                                                     const double4* __restrict__ pt, const double* __restrict__ p,
                                                     double* __restrict__ td, double* __restrict__ part) {
    if (st->stop) return;
    cg_dmf_ad_body(D, pt, p, td, part, blockIdx.x, gridDim.x);
}

// q += Adᵀ td by (y, x) node: a wave takes a strip of 64 nodes of one row (lane = node); each
// lane sums the points of its node's ≤ 4 cells (cell rows iy − 1, iy: two runs of the sorted
// order) in sorted order — weight of the corner the node is of each point's cell.  The 3-D part's
// column (t nodes) accumulates in LDS laid out [t][lane] (the t index varies per point; this
// layout is bank-conflict free whatever it is), then leaves as one contiguous run per strip.
// The strip's q values are loaded up front.
// ast (the CG step's q): workgroup 0 also computes α_k = ρ_k / pᵀNp from the normal and Ad·p
// kernels' partials (complete before this launch; this kernel does not read α) — one launch less
// per CG step than a separate k_cg_alpha.  st is then the same state: not __restrict__.
__device__ __forceinline__ void cg_alpha_body(CgState* st, const double* part_g, int ng, const double* part_t, int nt,
                                              const double* gsum);
// One node's sum over its points (the ≤ 4 cells around node (iy, ix): cell rows iy − 1, iy, in
// sorted order): returns the 2-D part's Σ w·td, and adds the 3-D part's column to acc[t·64].
__device__ __forceinline__ double dmf_node_gather(const DmfDesc& D, const int32_t* __restrict__ cell,
                                                  const double4* __restrict__ pt, const double* __restrict__ td, int iy,
                                                  int ix, double* __restrict__ acc) {
    const int C1 = D.S1 - 1;
    double a2 = 0.0;
    const bool r0 = iy >= 1, r1 = iy <= D.S0 - 2;
    const int ra = r0 ? (iy - 1) * C1 : 0, rb = r1 ? iy * C1 : 0;
    const int cxl = max(ix - 1, 0), cxh = min(ix, C1 - 1);
    const int a0 = r0 ? cell[ra + cxl] : 0, a1 = r0 ? cell[ra + cxh + 1] : 0;
    const int b0 = r1 ? cell[rb + cxl] : 0, b1 = r1 ? cell[rb + cxh + 1] : 0;
    const int na = a1 - a0, ntot = na + (b1 - b0);
    for (int j0 = 0; j0 < ntot; j0 += DMF_U) {
        double4 P[DMF_U];
        double tj[DMF_U];
#pragma unroll
        for (int u = 0; u < DMF_U; ++u) {
            const int j = j0 + u;
            const int idx = j < na ? a0 + j : b0 + (j - na);
            const bool in = j < ntot;
            P[u] = in ? pt[idx] : make_double4(0.0, 0.0, 0.0, 0.0);
            tj[u] = in ? td[idx] : 0.0;   // past the node's points: 0·w
        }
#pragma unroll
        for (int u = 0; u < DMF_U; ++u) {
            double fy, fx;
            const int pcy = dmf_cell(P[u].x, D.S0, fy), pcx = dmf_cell(P[u].y, D.S1, fx);
            const double wt = (pcy == iy ? 1.0 - fy : fy) * (pcx == ix ? 1.0 - fx : fx);
            a2 += wt * tj[u];
            if (D.n3) {
                double ft;
                const int ct = dmf_cell(P[u].z, D.S2, ft);
                acc[ct * 64] += (wt * (1.0 - ft)) * tj[u];
                acc[(ct + 1) * 64] += (wt * ft) * tj[u];
            }
        }
    }
    return a2;
}
template <int MT>   // register column length ≥ the 3-D part's t nodes (12 or CG_MAXT)
__global__ __launch_bounds__(BLOCK) void k_cg_dmf_atq(const CgState* st, DmfDesc D,
                                                      const int32_t* __restrict__ cell,
                                                      const double4* __restrict__ pt, const double* __restrict__ td,
                                                      double* __restrict__ q, CgState* ast, const double* apg, int ang,
                                                      const double* apt, int ant) {
    // the stop flag as this launch found it: workgroup 0's α body may set it (γ ≤ 0) while the
    // other workgroups — and the other waves of workgroup 0, which meet at the barrier below — read
    // it, so every wave reads it once, before the α body runs (with p = 0 the launch is a no-op)
    const int stopped = st->stop;
    if (ast && blockIdx.x == 0) cg_alpha_body(ast, apg, ang, apt, ant, nullptr);
    if (stopped) return;
    __shared__ double LA[BLOCK / 64][MT * 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nsx = (D.S1 + 63) / 64;
    const int64_t strip = (int64_t)xcd_block(blockIdx.x, gridDim.x) * (BLOCK / 64) + w;   // grid: a multiple of 8
    const bool live = strip < (int64_t)D.S0 * nsx;
    const int iy = live ? (int)(strip / nsx) : 0;
    const int x0 = live ? (int)(strip - (int64_t)iy * nsx) * 64 : 0;
    const int nv = live ? min(64, D.S1 - x0) : 0;
    double* __restrict__ qc = q + D.col3 + ((int64_t)iy * D.S1 + x0) * D.S2;
    double qv[MT], q2[2];
    if (D.n3) {
#pragma unroll
        for (int k = 0; k < MT; ++k) qv[k] = lane + 64 * k < nv * D.S2 ? qc[lane + 64 * k] : 0.0;
    }
    const int ix = x0 + lane;
    const bool mine = live && ix < D.S1;
    const int64_t nd = (int64_t)iy * D.S1 + ix;
#pragma unroll
    for (int k = 0; k < 2; ++k) q2[k] = mine && k < D.n2 ? q[D.col2[k] + nd] : 0.0;
    double* __restrict__ acc = &LA[w][lane];   // acc[t·64]
#pragma unroll
    for (int k = 0; k < MT; ++k) acc[k * 64] = 0.0;
    if (mine) {
        const double a2 = dmf_node_gather(D, cell, pt, td, iy, ix, acc);
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (k < D.n2) q[D.col2[k] + nd] = q2[k] + a2;
    }
    if (D.n3) {
        __syncthreads();   // every lane's column is complete
        const int S2 = D.S2;
        const double* __restrict__ L = LA[w];
#pragma unroll
        for (int k = 0; k < MT; ++k) {
            const int e = lane + 64 * k;
            if (e < nv * S2) {
                const int nl = e / S2;
                qc[e] = qv[k] + L[(e - nl * S2) * 64 + nl];
            }
        }
    }
}

// dmf_node_gather for one chunk [t0, t0 + tlen) of the node's column: every point of the node is
// walked in the same sorted order and adds the corners of its t cell that fall inside the chunk to
// acc[(t − t0)·64], so each entry of the column receives the terms, and the order, it has there.
__device__ __forceinline__ double dmf_node_gather_chunk(const DmfDesc& D, const int32_t* __restrict__ cell,
                                                        const double4* __restrict__ pt, const double* __restrict__ td,
                                                        int iy, int ix, int t0, int tlen, double* __restrict__ acc) {
    const int C1 = D.S1 - 1;
    double a2 = 0.0;
    const bool r0 = iy >= 1, r1 = iy <= D.S0 - 2;
    const int ra = r0 ? (iy - 1) * C1 : 0, rb = r1 ? iy * C1 : 0;
    const int cxl = max(ix - 1, 0), cxh = min(ix, C1 - 1);
    const int a0 = r0 ? cell[ra + cxl] : 0, a1 = r0 ? cell[ra + cxh + 1] : 0;
    const int b0 = r1 ? cell[rb + cxl] : 0, b1 = r1 ? cell[rb + cxh + 1] : 0;
    const int na = a1 - a0, ntot = na + (b1 - b0);
    for (int j0 = 0; j0 < ntot; j0 += DMF_U) {
        double4 P[DMF_U];
        double tj[DMF_U];
#pragma unroll
        for (int u = 0; u < DMF_U; ++u) {
            const int j = j0 + u;
            const int idx = j < na ? a0 + j : b0 + (j - na);
            const bool in = j < ntot;
            P[u] = in ? pt[idx] : make_double4(0.0, 0.0, 0.0, 0.0);
            tj[u] = in ? td[idx] : 0.0;   // past the node's points: 0·w
        }
#pragma unroll
        for (int u = 0; u < DMF_U; ++u) {
            double fy, fx, ft;
            const int pcy = dmf_cell(P[u].x, D.S0, fy), pcx = dmf_cell(P[u].y, D.S1, fx);
            const double wt = (pcy == iy ? 1.0 - fy : fy) * (pcx == ix ? 1.0 - fx : fx);
            a2 += wt * tj[u];
            const int tl = dmf_cell(P[u].z, D.S2, ft) - t0;   // the cell's lower corner, chunk-relative
            if (tl >= 0 && tl < tlen) acc[tl * 64] += (wt * (1.0 - ft)) * tj[u];
            if (tl >= -1 && tl + 1 < tlen) acc[(tl + 1) * 64] += (wt * ft) * tj[u];
        }
    }
    return a2;
}

// k_cg_dmf_atq for a 3-D part of CG_MAXT < S2 ≤ DMF_MAXT_LONG t nodes (lsq_set_cg_tile_dmf).  A whole
// column per lane no longer fits LA (64 t × 64 lanes × 8 B = 32 KB a wave), so the column is cut into
// nch = ⌈S2 / DMF_TC⌉ chunks of near-equal length ≤ DMF_TC and a wave takes one (strip, chunk): it
// walks all the points of its lanes' nodes and keeps the corners that fall in its chunk
// (dmf_node_gather_chunk).  The chunks of a strip sit in consecutive waves (of one workgroup when
// nch = 4 or 2), so the points' second to fourth reads hit the vector L1; LDS stays 32 KB a
// workgroup and the occupancy that of k_cg_dmf_atq<CG_MAXT> (DESIGN.md §3).  Chunk 0's wave also
// adds the 2-D parts' sum.  Same sums in the same order as one wave per whole column would give.
__global__ __launch_bounds__(BLOCK) void k_cg_dmf_atq_long(const CgState* st, DmfDesc D,
                                                           const int32_t* __restrict__ cell,
                                                           const double4* __restrict__ pt,
                                                           const double* __restrict__ td, double* __restrict__ q,
                                                           CgState* ast, const double* apg, int ang, const double* apt,
                                                           int ant) {
    const int stopped = st->stop;   // as k_cg_dmf_atq: read once, before workgroup 0's α body may set it
    if (ast && blockIdx.x == 0) cg_alpha_body(ast, apg, ang, apt, ant, nullptr);
    if (stopped) return;
    __shared__ double LA[BLOCK / 64][DMF_TC * 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int S2 = D.S2, nsx = (D.S1 + 63) / 64, nch = (S2 + DMF_TC - 1) / DMF_TC;
    const int64_t unit = (int64_t)xcd_block(blockIdx.x, gridDim.x) * (BLOCK / 64) + w;   // grid: a multiple of 8
    const bool live = unit < (int64_t)D.S0 * nsx * nch;
    const int64_t strip = live ? unit / nch : 0;
    const int ck = live ? (int)(unit - strip * nch) : 0;
    const int t0 = ck * S2 / nch, tlen = live ? (ck + 1) * S2 / nch - t0 : 0;   // ≤ DMF_TC nodes
    const int iy = (int)(strip / nsx);
    const int x0 = (int)(strip - (int64_t)iy * nsx) * 64;
    const int nv = live ? min(64, D.S1 - x0) : 0;
    double* __restrict__ qc = q + D.col3 + ((int64_t)iy * D.S1 + x0) * S2 + t0;   // entry (node nl, t0 + tt): qc[nl·S2 + tt]
    double qv[DMF_TC], q2[2];
    // the lane's entries e = lane + 64k of the chunk's nv × tlen: node nl = ⌊e / tlen⌋ = (e·rt) >> 16
    // (exact: e < 1024, tlen ≤ 16, so e·(rt·tlen − 2¹⁶) < 2¹⁶)
    const int rt = tlen ? (65536 + tlen - 1) / tlen : 0;
#pragma unroll
    for (int k = 0; k < DMF_TC; ++k) {
        const int e = lane + 64 * k;
        const int nl = (e * rt) >> 16;
        qv[k] = e < nv * tlen ? qc[nl * S2 + (e - nl * tlen)] : 0.0;
    }
    const int ix = x0 + lane;
    const bool mine = live && ix < D.S1;
    const int64_t nd = (int64_t)iy * D.S1 + ix;
    const bool two = mine && ck == 0;   // the 2-D parts leave with the strip's first chunk
#pragma unroll
    for (int k = 0; k < 2; ++k) q2[k] = two && k < D.n2 ? q[D.col2[k] + nd] : 0.0;
    double* __restrict__ acc = &LA[w][lane];   // acc[(t − t0)·64]
#pragma unroll
    for (int k = 0; k < DMF_TC; ++k) acc[k * 64] = 0.0;
    if (mine) {
        const double a2 = dmf_node_gather_chunk(D, cell, pt, td, iy, ix, t0, tlen, acc);
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (two && k < D.n2) q[D.col2[k] + nd] = q2[k] + a2;
    }
    __syncthreads();   // every lane's chunk is complete
    const double* __restrict__ L = LA[w];
#pragma unroll
    for (int k = 0; k < DMF_TC; ++k) {
        const int e = lane + 64 * k;
        if (e < nv * tlen) {
            const int nl = (e * rt) >> 16, tt = e - nl * tlen;
            qc[nl * S2 + tt] = qv[k] + L[tt * 64 + nl];
        }
    }
}

// row scales of the data rows in sorted point order (once per solve: weights change between solves)
__global__ __launch_bounds__(BLOCK) void k_dmf_rs(int64_t npts, const int32_t* __restrict__ perm,
                                                  const double* __restrict__ rs, double4* __restrict__ pt) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < npts; i += (int64_t)gridDim.x * BLOCK)
        pt[i].w = rs[perm[i]];
}

// CG's s0 = Aᵀ(W b) when x0 = 0 and b vanishes past the data rows (a cold smooth_fit solve): u = W b
// lives on the data rows only, so per sorted point td = w·(w b) (the row scale twice, as the CG
// step's td) for the node gather, and the partials of ‖W b‖² (= ‖r0‖²)
__global__ __launch_bounds__(BLOCK) void k_cg_init_dmf(int64_t npts, const int32_t* __restrict__ perm,
                                                       const double4* __restrict__ pt, const double* __restrict__ b,
                                                       double* __restrict__ td, double* __restrict__ part) {
    double ss = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < npts; i += (int64_t)gridDim.x * BLOCK) {
        const double w = pt[i].w, u = w * b[perm[i]];
        td[i] = w * u;
        ss += u * u;
    }
    store_partial(ss, part, blockIdx.x);
}

// ---- column mode: strips streamed through an LDS ring ----------------------------------------
// A workgroup owns a STRIP: CG_TX dim-1 positions × ys..ye rows of dim 0 × all of dim 2.  It
// walks the strip RS = 4·rpw rows per step through a ring of R = RS + 2·hy staged rows (row y
// at slot (y − ys + hy) mod R, image front + slot·rowimg + xi·tpad + t): while the waves
// compute the step's rows from the ring, the next RS rows of z and p_old are already in flight
// into registers; they replace the ring rows no longer needed after a barrier.  Every p value
// is staged once per strip (plus the 2·hy halo rows per strip).

// Staging map (wave rows): wave w stages rows w, w + 4, … of every block of RS rows; lane l owns
// the row-image columns c = l + 64k (k < NCW: dim-1 position xi = c / tpad, dim-2 position
// t = c mod tpad), decomposed once per strip.  A wave's staged row is the one whose ring slot it
// frees, so the q staging and the refill of that slot need no workgroup barrier between them.
template <int NCW>
struct CgWCols {
    int32_t goff[NCW];   // (x0 − hx + xi)·S2 + t, or -1 (outside the grid / dim-2 padding / image)
    uint32_t own;        // bit k: inside the strip's CG_TX positions and the grid
};

// cs / co: the lane owns columns lane + 64·(cs·k + co) (cs = 2: a wave stages half a row image,
// its partner wave the other half — the 8-wave column kernel)
template <int NCW>
__device__ __forceinline__ void cg_wcols_init(const CgGrid& C, int x0, int lane, CgWCols<NCW>& cc, int cs = 1,
                                              int co = 0) {
    const int rowimg = C.wx * C.tpad;
    cc.own = 0;
#pragma unroll
    for (int k = 0; k < NCW; ++k) {
        const int c = lane + 64 * (cs * k + co);
        const int xi = (int)fdiv((uint32_t)c, C.fd_pad);
        const int t = c - xi * C.tpad, x = x0 - C.hx + xi;
        const bool ok = c < rowimg && t < C.shape[2] && x >= 0 && x < C.shape[1];
        cc.goff[k] = ok ? x * C.shape[2] + t : -1;
        if (ok && xi >= C.hx && xi < C.hx + CG_TX) cc.own |= 1u << k;
    }
}

// z, p_old of this wave's rows yb + wid + 4k (k < RPW, row index < nrows) into registers
template <int RPW, int NCW, int NW = 4>
__device__ __forceinline__ void cg_wload(const CgGrid& C, const CgWCols<NCW>& cc, int yb, int nrows, int wid,
                                         const double* __restrict__ z, const double* __restrict__ pold,
                                         double (&zr)[RPW][NCW], double (&pr)[RPW][NCW]) {
    const int64_t rowlen = (int64_t)C.shape[1] * C.shape[2];
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int r = wid + NW * k, y = yb + r;
        const bool rok = r < nrows && y >= 0 && y < C.shape[0];
        const int64_t base = C.col0 + (int64_t)y * rowlen;
#pragma unroll
        for (int j = 0; j < NCW; ++j) {
            const bool ok = rok && cc.goff[j] >= 0;
            zr[k][j] = ok ? z[base + cc.goff[j]] : 0.0;
            pr[k][j] = ok && pold ? pold[base + cc.goff[j]] : 0.0;   // multigrid ops: no p_old
        }
    }
}

// p = z + β p_old of this wave's rows into their ring slots ((y − ys + hy) mod R); rows of
// [ys, ye) inside the strip's CG_TX positions also go to pnew
template <int RPW, int NCW, int NW = 4>
__device__ __forceinline__ void cg_wstore(const CgGrid& C, const CgWCols<NCW>& cc, int yb, int nrows, int wid,
                                          int lane, int ys, int ye, int R, double beta,
                                          const double (&zr)[RPW][NCW], const double (&pr)[RPW][NCW], double* L,
                                          double* __restrict__ pnew, int cs = 1, int co = 0) {
    const int rowimg = C.wx * C.tpad;
    const int64_t rowlen = (int64_t)C.shape[1] * C.shape[2];
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int r = wid + NW * k, y = yb + r;
        if (r >= nrows) continue;
        const int slot = (y - ys + C.hy) % R;
        const bool own_row = y >= ys && y < ye;
        const int64_t base = C.col0 + (int64_t)y * rowlen;
#pragma unroll
        for (int j = 0; j < NCW; ++j) {
            const int c = lane + 64 * (cs * j + co);
            const double v = zr[k][j] + beta * pr[k][j];
            if (c < rowimg) L[C.front + slot * rowimg + c] = v;
            if (pnew && own_row && (cc.own >> j & 1u)) pnew[base + cc.goff[j]] = v;
        }
    }
}

// Column mode: the groups of one dt width for the column of row slot `srow` (t = 0 at
// front + srow·rowimg + cb): acc[t] += Σ_g Σ_d cf[g][t][d] · p(y + dy_g, x + dx_g, t + d − DT).
// cf is wave-uniform in the XUNI instantiation (scalar loads), per lane otherwise.
// t0: the first epoch of the column this lane accumulates (0, or the second half's start in the
// 8-wave column kernel: acc[t] is epoch t0 + t)
template <int MAXT, int DT>
__device__ __forceinline__ void cg_col_groups(const CgGrid& C, const double* __restrict__ cf0,
                                              const double* __restrict__ L, int srow, int R, int cb, int g0, int ng,
                                              double (&acc)[MAXT], int t0 = 0) {
    constexpr int W = 2 * DT + 1;
    const int rowimg = C.wx * C.tpad;
    for (int g = g0; g < g0 + ng; ++g) {
        int slot = srow + C.gdy[g];
        slot += slot < 0 ? R : 0;
        slot -= slot >= R ? R : 0;
        const int lo = C.front + slot * rowimg + cb + C.gl[g] - DT + t0;
        const double* __restrict__ cf = cf0 + C.gc[g] + t0 * W;
        double cv[MAXT + 2 * DT];
#pragma unroll
        for (int j = 0; j < MAXT + 2 * DT; ++j) cv[j] = L[lo + j];   // t ≥ S2 taps have zero coefficients
#pragma unroll
        for (int t = 0; t < MAXT; ++t)
#pragma unroll
            for (int d = 0; d < W; ++d) acc[t] += cf[t * W + d] * cv[t + d];
    }
}

// Column mode: N_s p for the column (y, x0 + lane, ·) whose row sits at ring slot srow, with the
// coefficients of the interior dim-1 class (wave-uniform: scalar loads); nodes of the dim-1 edge
// classes are corrected by k_cg_xedge.  acc = N_s p, gam += p·(N_s p).
template <int MAXT>
__device__ __forceinline__ void cg_col_row(const CgGrid& C, const double* __restrict__ coef,
                                           const double* __restrict__ L, int y, int srow, int R, int x0, int lane,
                                           double (&acc)[MAXT], double& gam, int dbg, int t0 = 0) {
    const int S2 = MAXT == 1 ? 1 : C.shape[2] - t0;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) acc[t] = 0.0;
    const int cy = cg_cls(y, C.shape[0], C.K[0], C.ncls[0]);
    const int rb = __builtin_amdgcn_readfirstlane(C.coefc0 + (cy * C.ncls[1] + C.K[1]) * C.rowlen);
    const double* __restrict__ cf0 = coef + rb;
    const int cb = (lane + C.hx) * C.tpad;
    const int n0 = (dbg & 1) ? 0 : C.ngrp[0], n1 = (dbg & 1) ? 0 : C.ngrp[1], n2 = (dbg & 1) ? 0 : C.ngrp[2];
    if (n0) cg_col_groups<MAXT, 0>(C, cf0, L, srow, R, cb, 0, n0, acc, t0);
    if (MAXT > 1 && n1) cg_col_groups<MAXT, 1>(C, cf0, L, srow, R, cb, n0, n1, acc, t0);
    if (MAXT > 1 && n2) cg_col_groups<MAXT, 2>(C, cf0, L, srow, R, cb, n0 + n1, n2, acc, t0);
    if (x0 + lane < C.shape[1]) {
        const int c0 = C.front + srow * C.wx * C.tpad + cb + t0;
#pragma unroll
        for (int t = 0; t < MAXT; ++t)
            if (t < S2) gam += L[c0 + t] * acc[t];
    }
}

// q = acc for one row of the strip, through a wave-private LDS area (lane-major, stride tpad) so
// the row's CG_TX·S2 consecutive values are stored with coalesced accesses
template <int MAXT>
__device__ __forceinline__ void cg_col_store(const CgGrid& C, double* Lw, int y, int x0, int lane,
                                             const double (&acc)[MAXT], double* __restrict__ q, int dbg) {
    const int S1 = C.shape[1], S2 = MAXT == 1 ? 1 : C.shape[2];
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
        if (t < S2) Lw[lane * C.tpad + t] = acc[t];
    if (dbg & 2) return;
    const int nx = min(CG_TX, S1 - x0), n = nx * S2;
    const int64_t off = ((int64_t)y * S1 + x0) * S2;
#pragma unroll
    for (int k = 0; k < MAXT; ++k) {
        const int j = lane + 64 * k;
        if (j < n) {
            const int xi = MAXT == 1 ? j : (int)fdiv((uint32_t)j, C.fd_s2);
            const int t = j - xi * S2;
            q[C.col0 + off + j] = Lw[xi * C.tpad + t];
        }
    }
}

template <int MAXT, int RPW, int NCW, int NW = 4>
__device__ __forceinline__ void cg_strip_step(const CgGrid& C, const double* __restrict__ coef, double* __restrict__ q,
                                              double* L, int ys, int ye, int y, int R, int x0, int lane, int wid,
                                              double& gam, int dbg) {
    constexpr int RS = NW * RPW;
    const int rowimg = C.wx * C.tpad;
    double acc[RPW][MAXT];
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int yy = y + wid + NW * k;
        if (yy < ye) cg_col_row<MAXT>(C, coef, L, yy, (yy - ys + C.hy) % R, R, x0, lane, acc[k], gam, dbg);
    }
    __syncthreads();   // ring rows y − hy .. y − hy + RS − 1 are free
    // each wave: q of its rows staged through the slot of row y − hy + wid + 4k, which is then
    // refilled with row y + RS + hy + wid + 4k by the caller (same slot: the two differ by R rows)
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int yy = y + wid + NW * k;
        double* Lw = L + C.front + ((y - ys + wid + NW * k) % R) * rowimg;
        if (yy < ye) cg_col_store<MAXT>(C, Lw, yy, x0, lane, acc[k], q, dbg);
    }
    (void)RS;
}

// A strip streams its rows through the ring: one row block of z / p_old in flight in registers,
// loaded at the start of the step whose end it refills.  (Two blocks in flight, alternating by
// step, measured slower: C4 ring kernel 166–170 → 231 µs, the wider register set; no gain on a
// 130-row slab.)
template <int MAXT, int RPW, int NCW, int NW = 4>
__device__ __forceinline__ void cg_strip(const CgGrid& C, const double* __restrict__ coef, double beta,
                                         const double* __restrict__ z, const double* __restrict__ pold,
                                         double* __restrict__ pnew, double* __restrict__ q, double* L, int ys, int ye,
                                         int x0, double& gam, int dbg) {
    constexpr int RS = NW * RPW;
    const int hy = C.hy, R = RS + 2 * hy, rowimg = C.wx * C.tpad;
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if ((int)threadIdx.x < C.front) L[threadIdx.x] = 0.0;   // pads read (× 0) by the edge taps
    for (int i = threadIdx.x; i < C.lds - C.front - R * rowimg; i += NW * 64) L[C.lds - 1 - i] = 0.0;
    CgWCols<NCW> cc;
    cg_wcols_init<NCW>(C, x0, lane, cc);
    double zr[RPW][NCW], pr[RPW][NCW];
    {   // prologue: rows ys − hy .. ys + RS + hy − 1; the first two row blocks in flight together
        double zr2[RPW][NCW], pr2[RPW][NCW];
        const int y1 = ys - hy + RS, n2 = min(RS, ys + RS + hy - y1);
        cg_wload<RPW, NCW, NW>(C, cc, ys - hy, RS, wid, z, pold, zr, pr);
        cg_wload<RPW, NCW, NW>(C, cc, y1, n2, wid, z, pold, zr2, pr2);
        cg_wstore<RPW, NCW, NW>(C, cc, ys - hy, RS, wid, lane, ys, ye, R, beta, zr, pr, L, pnew);
        cg_wstore<RPW, NCW, NW>(C, cc, y1, n2, wid, lane, ys, ye, R, beta, zr2, pr2, L, pnew);
        for (int yb = y1 + RS; yb < ys + RS + hy; yb += RS) {   // halo deeper than RS / 2
            const int nr = min(RS, ys + RS + hy - yb);
            cg_wload<RPW, NCW, NW>(C, cc, yb, nr, wid, z, pold, zr, pr);
            cg_wstore<RPW, NCW, NW>(C, cc, yb, nr, wid, lane, ys, ye, R, beta, zr, pr, L, pnew);
        }
    }
    __syncthreads();
    for (int y = ys; y < ye; y += RS) {
        const bool more = y + RS < ye;
        if (more && !(dbg & 4)) cg_wload<RPW, NCW, NW>(C, cc, y + RS + hy, RS, wid, z, pold, zr, pr);   // in flight
        cg_strip_step<MAXT, RPW, NCW, NW>(C, coef, q, L, ys, ye, y, R, x0, lane, wid, gam, dbg);
        if (more) cg_wstore<RPW, NCW, NW>(C, cc, y + RS + hy, RS, wid, lane, ys, ye, R, beta, zr, pr, L, pnew);
        __syncthreads();
    }
}

// 8-wave column kernel, grids with more than one node along dim 2: waves w and w + 4 share ring
// row w of each step, wave w + 4·h staging the columns lane + 64·(2k + h) of its rows and
// accumulating the epochs 6h .. 6h + 5 of its column (t0 = 6h); q leaves straight from the
// registers (6 consecutive epochs per lane).  Same ring, same LDS as the 4-wave kernel: 16 waves
// per CU instead of 8 (the 4-wave kernel is latency-bound: DESIGN.md §8).
template <int NCWH>
__device__ __forceinline__ void cg_strip_th(const CgGrid& C, const double* __restrict__ coef, double beta,
                                            const double* __restrict__ z, const double* __restrict__ pold,
                                            double* __restrict__ pnew, double* __restrict__ q, double* L, int ys,
                                            int ye, int x0, double& gam, int dbg) {
    constexpr int RS = 4, NT = 6;
    const int hy = C.hy, R = RS + 2 * hy, rowimg = C.wx * C.tpad;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wid = wv & 3, half = wv >> 2, t0 = NT * half;
    if ((int)threadIdx.x < C.front) L[threadIdx.x] = 0.0;
    for (int i = threadIdx.x; i < C.lds - C.front - R * rowimg; i += 512) L[C.lds - 1 - i] = 0.0;
    CgWCols<NCWH> cc;
    cg_wcols_init<NCWH>(C, x0, lane, cc, 2, half);
    double zr[1][NCWH], pr[1][NCWH];
    {
        double zr2[1][NCWH], pr2[1][NCWH];
        const int y1 = ys - hy + RS, n2 = min(RS, ys + RS + hy - y1);
        cg_wload<1, NCWH>(C, cc, ys - hy, RS, wid, z, pold, zr, pr);
        cg_wload<1, NCWH>(C, cc, y1, n2, wid, z, pold, zr2, pr2);
        cg_wstore<1, NCWH>(C, cc, ys - hy, RS, wid, lane, ys, ye, R, beta, zr, pr, L, pnew, 2, half);
        cg_wstore<1, NCWH>(C, cc, y1, n2, wid, lane, ys, ye, R, beta, zr2, pr2, L, pnew, 2, half);
        for (int yb = y1 + RS; yb < ys + RS + hy; yb += RS) {
            const int nr = min(RS, ys + RS + hy - yb);
            cg_wload<1, NCWH>(C, cc, yb, nr, wid, z, pold, zr, pr);
            cg_wstore<1, NCWH>(C, cc, yb, nr, wid, lane, ys, ye, R, beta, zr, pr, L, pnew, 2, half);
        }
    }
    __syncthreads();
    const int S1 = C.shape[1], S2 = C.shape[2], x = x0 + lane;
    for (int y = ys; y < ye; y += RS) {
        const bool more = y + RS < ye;
        if (more && !(dbg & 4)) cg_wload<1, NCWH>(C, cc, y + RS + hy, RS, wid, z, pold, zr, pr);
        const int yy = y + wid;
        double acc[NT];
        if (yy < ye) cg_col_row<NT>(C, coef, L, yy, (yy - ys + hy) % R, R, x0, lane, acc, gam, dbg, t0);
        if (yy < ye && x < S1 && !(dbg & 2)) {
            double* qr = q + C.col0 + ((int64_t)yy * S1 + x) * S2 + t0;
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (t0 + t < S2) qr[t] = acc[t];
        }
        __syncthreads();   // ring rows y − hy .. y − hy + RS − 1 are free
        if (more) cg_wstore<1, NCWH>(C, cc, y + RS + hy, RS, wid, lane, ys, ye, R, beta, zr, pr, L, pnew, 2, half);
        __syncthreads();
    }
}

// Column-mode normal operator: workgroup b processes strip b (y rows ys..ys+ty−1, dim-1
// positions x0..x0+CG_TX−1) of every grid in turn (same strip grid for all), through the LDS
// ring above.  q = N_s p (the stencil rows' share; the update kernel adds ATd·t), p = z + β p_old
// written once; gam partial = pᵀN_s p (the data share ‖t‖² = ‖Ad p‖² comes from k_cg_data).
// Multigrid level operators (mg.inc) call it with p_old and/or pnew null and β from betap.
template <int MAXT3>   // register column length of the grids with more than one node along dim 2
__global__ __launch_bounds__(BLOCK) void k_cg_normal_col(const CgState* __restrict__ st, const CgDesc* __restrict__ cd,
                                                         const double* __restrict__ coef, const double* __restrict__ z,
                                                         const double* __restrict__ pold, double* __restrict__ pnew,
                                                         double* __restrict__ q, double* __restrict__ part,
                                                         const double* __restrict__ betap) {
    if (st->stop) return;
    const int tile = cg_tile_of_block();
    double gam = 0.0;
    if (tile < cd->ntiles) {
        double* L = mf_zl;
        const double beta = betap ? *betap : st->beta;   // multigrid ops pass their own scalar
        const int dbg = cd->colmode >> 1;
        bool first = true;
        for (int g = 0; g < cd->n_grids; ++g) {
            const CgGrid& C = cd->g[g];
            if (!C.noff || tile >= C.nty * C.ntx) continue;
            if (!first) __syncthreads();   // the previous grid's ring is no longer read
            first = false;
            const int tyi = tile / C.ntx;
            const int ys = tyi * C.ty, ye = min(ys + C.ty, C.shape[0]), x0 = (tile - tyi * C.ntx) * CG_TX;
            if (C.maxt == 1) cg_strip<1, 4, 2>(C, coef, beta, z, pold, pnew, q, L, ys, ye, x0, gam, dbg);
            else cg_strip<MAXT3, 1, CG_NCW>(C, coef, beta, z, pold, pnew, q, L, ys, ye, x0, gam, dbg);
        }
    }
    store_partial(gam, part, blockIdx.x);
}

// The 8-wave variant of k_cg_normal_col (the CG iteration's operator, LSQ_CG_W8): 3-D grids of
// ≤ 12 epochs by the t-split strip, 2-D grids by the plain strip with 8 waves of 2 rows each (the
// same RS = 16 ring).  Workgroups of 512 threads, the same dynamic LDS.
__global__ __launch_bounds__(512) void k_cg_normal_col8(const CgState* __restrict__ st, const CgDesc* __restrict__ cd,
                                                        const double* __restrict__ coef, const double* __restrict__ z,
                                                        const double* __restrict__ pold, double* __restrict__ pnew,
                                                        double* __restrict__ q, double* __restrict__ part,
                                                        const double* __restrict__ betap) {
    if (st->stop) return;
    const int tile = cg_tile_of_block();
    double gam = 0.0;
    if (tile < cd->ntiles) {
        double* L = mf_zl;
        const double beta = betap ? *betap : st->beta;   // multigrid ops pass their own scalar
        const int dbg = cd->colmode >> 1;
        bool first = true;
        for (int g = 0; g < cd->n_grids; ++g) {
            const CgGrid& C = cd->g[g];
            if (!C.noff || tile >= C.nty * C.ntx) continue;
            if (!first) __syncthreads();
            first = false;
            const int tyi = tile / C.ntx;
            const int ys = tyi * C.ty, ye = min(ys + C.ty, C.shape[0]), x0 = (tile - tyi * C.ntx) * CG_TX;
            if (C.maxt == 1) cg_strip<1, 2, 2, 8>(C, coef, beta, z, pold, pnew, q, L, ys, ye, x0, gam, dbg);
            else cg_strip_th<CG_NCW / 2>(C, coef, beta, z, pold, pnew, q, L, ys, ye, x0, gam, dbg);
        }
    }
    __shared__ double red[8];   // store_partial for 8 waves
    const double v = wave_sum(gam);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        part[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
}

#include "lsqr_cg_rw.inc"

// Column mode, dim-1 edge correction: for nodes whose dim-1 class is not the interior one,
// q += (N_class − N_interior) p over the tile-mode offset table (class rows incl. dim 2), p from
// pnew; partial Σ p·Δq into part.  One thread per (grid, row, edge position, t) item.
// XE_LPC lanes per item: offsets strided over the lanes (8: short gather chains — the CG
// iteration, beside the data rows, and the multigrid levels; 1: LSQ_CG_XE=1)
template <int XE_LPC>
__device__ __forceinline__ void cg_xedge_body(const CgDesc* __restrict__ cd, const double* __restrict__ coef,
                                              const double* __restrict__ p, double* __restrict__ q,
                                              double* __restrict__ part, int bid) {
    double gam = 0.0;
    const int sub = threadIdx.x % XE_LPC;
    int64_t i = ((int64_t)bid * BLOCK + threadIdx.x) / XE_LPC;
    for (int g = 0; g < cd->n_grids; ++g) {
        const CgGrid& C = cd->g[g];
        if (!C.noff) continue;
        const int S0 = C.shape[0], S1 = C.shape[1], S2 = C.shape[2];
        const int K1 = C.K[1], ne = C.ncls[1] == S1 ? S1 : 2 * K1;   // edge positions per row
        const int64_t items = (int64_t)S0 * ne * S2;
        if (i >= items) {
            i -= items;
            continue;
        }
        const int t = (int)(i % S2);
        const int64_t r = i / S2;
        const int e = (int)(r % ne), y = (int)(r / ne);
        const int x = C.ncls[1] == S1 ? e : (e < K1 ? e : S1 - 2 * K1 + e);
        const int cy = cg_cls(y, S0, C.K[0], C.ncls[0]), cx = cg_cls(x, S1, K1, C.ncls[1]);
        const int ct = cg_cls(t, S2, C.K[2], C.ncls[2]);
        if (cx == K1) break;   // tiny grids: the interior class itself (all lanes of the item)
        const double* __restrict__ ce = coef + C.coef0 + ((cy * C.ncls[1] + cx) * C.ncls[2] + ct) * C.noff;
        const double* __restrict__ ci = coef + C.coef0 + ((cy * C.ncls[1] + K1) * C.ncls[2] + ct) * C.noff;
        const int64_t c = C.col0 + ((int64_t)y * S1 + x) * S2 + t;
        double dq = 0.0;
        // the item's XE_LPC lanes take every XE_LPC-th offset (short gather chains), branch-free
        // (outside taps: coefficient 0 on the node itself), then a fixed shuffle tree
        for (int o = sub; o < C.noff; o += XE_LPC) {
            const int yy = y + C.ooff[o][0], xx = x + C.ooff[o][1], tt = t + C.ooff[o][2];
            const bool ok = yy >= 0 && yy < S0 && xx >= 0 && xx < S1 && tt >= 0 && tt < S2;
            const int64_t j = ok ? C.col0 + ((int64_t)yy * S1 + xx) * S2 + tt : c;
            dq += (ok ? ce[o] - ci[o] : 0.0) * p[j];
        }
#pragma unroll
        for (int m = XE_LPC / 2; m >= 1; m /= 2) dq += __shfl_xor(dq, m, XE_LPC);
        if (sub == 0) {
            q[c] += dq;
            gam += p[c] * dq;
        }
        break;
    }
    store_partial(gam, part, bid);
}

template <int XE_LPC>
__global__ __launch_bounds__(BLOCK) void k_cg_xedge(const CgState* __restrict__ st, const CgDesc* __restrict__ cd,
                                                    const double* __restrict__ coef, const double* __restrict__ p,
                                                    double* __restrict__ q, double* __restrict__ part) {
    if (st->stop) return;
    cg_xedge_body<XE_LPC>(cd, coef, p, q, part, blockIdx.x);
}

// t = Ad·p (workgroups [0, gD)) and the x-edge correction of q (the rest) in one launch: both read
// only p, and a second stream for the edge items cost more in fork/join gaps (about 17 µs per
// operator application at C4) than the launch it saved
template <int XE_LPC>
__global__ __launch_bounds__(BLOCK) void k_cg_ad_xedge(const CgState* __restrict__ st, DmfDesc D,
                                                       const double4* __restrict__ pt, const double* __restrict__ p,
                                                       double* __restrict__ td, double* __restrict__ part_t, int gD,
                                                       const CgDesc* __restrict__ cd, const double* __restrict__ coef,
                                                       double* __restrict__ q, double* __restrict__ part_e) {
    if (st->stop) return;
    if ((int)blockIdx.x < gD) cg_dmf_ad_body(D, pt, p, td, part_t, blockIdx.x, gD);
    else cg_xedge_body<XE_LPC>(cd, coef, p, q, part_e, (int)blockIdx.x - gD);
}

// ATD = false (lsq_set_cg_tile_dmf): q = N_s p alone; the matrix-free data rows add theirs behind this
// launch (k_cg_dmf_ad, the elimination, the node gather), and arp, aci, aval, td are not read
template <bool ATD = true>
__global__ __launch_bounds__(BLOCK) void k_cg_normal(const CgState* __restrict__ st, const CgDesc* __restrict__ cd,
                                                     const double* __restrict__ coef, const double* __restrict__ z,
                                                     const double* __restrict__ pold, double* __restrict__ pnew,
                                                     double* __restrict__ q, const int32_t* __restrict__ arp,
                                                     const int32_t* __restrict__ aci, const double* __restrict__ aval,
                                                     const double* __restrict__ td, double* __restrict__ part) {
    if (st->stop) return;
    const int tile = cg_tile_of_block();
    if (tile >= cd->ntiles) {
        if (threadIdx.x == 0) part[blockIdx.x] = 0.0;
        return;
    }
    int g = 0;
    while (g + 1 < cd->n_grids && tile >= cd->g[g + 1].tile0) ++g;   // tiles are numbered grid by grid
    const CgGrid& C = cd->g[g];
    const int tl = tile - C.tile0;
    const int tyi = tl / C.ntx;
    const int y0 = tyi * C.ty, x0 = (tl - tyi * C.ntx) * CG_TX;
    const int S0 = C.shape[0], S1 = C.shape[1], S2 = C.shape[2];
    const int hy = C.hy, hx = C.hx, wx = C.wx, tpad = C.tpad, front = C.front;
    const int64_t col0 = C.col0;
    const double beta = st->beta;
    double* L = mf_zl;

    // 1. stage p = z + β p_old over the tile and its halo
    cg_stage_p(C, y0, x0, beta, z, pold, pnew, L);
    __syncthreads();

    // 2. q = N p (+ the data rows' Adᵀt) for the tile's nodes: lane = dim-1 position, a wave
    //    takes (row, dim-2) items wid, wid+4, ...; the coefficient row is wave-uniform (scalar
    //    loads) unless the tile touches a dim-1 edge
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nitems = C.ty * S2;
    const int x = x0 + lane;
    const bool xin = x < S1;
    const int cx = cg_cls(xin ? x : 0, S1, C.K[1], C.ncls[1]);
    const bool xuni = x0 >= C.K[1] && x0 + CG_TX - 1 <= S1 - 1 - C.K[1];
    const int noff = C.noff;
    double qv[CG_MAXI];
    double gam = 0.0;
#pragma unroll
    for (int k = 0; k < CG_MAXI; ++k) {
        qv[k] = 0.0;
        const int it = wid + 4 * k;
        if (it >= nitems) continue;
        const int tyl = it / S2, t = it - tyl * S2;
        const int y = y0 + tyl;
        if (y >= S0) continue;
        const int cy = cg_cls(y, S0, C.K[0], C.ncls[0]), ct = cg_cls(t, S2, C.K[2], C.ncls[2]);
        const int center = front + ((tyl + hy) * wx + lane + hx) * tpad + t;
        double acc = 0.0;
        if (xuni) {
            const int rb = __builtin_amdgcn_readfirstlane(C.coef0 + ((cy * C.ncls[1] + C.K[1]) * C.ncls[2] + ct) * noff);
            const double* __restrict__ cr = coef + rb;
            for (int o = 0; o < noff; ++o) acc += cr[o] * L[center + C.loff[o]];
        } else {
            const double* __restrict__ cr = coef + C.coef0 + ((cy * C.ncls[1] + cx) * C.ncls[2] + ct) * noff;
            for (int o = 0; o < noff; ++o) acc += cr[o] * L[center + C.loff[o]];
        }
        if (xin) {
            if (ATD) {
                const int64_t pos = (int64_t)C.node0 + ((int64_t)y * S1 + x) * S2 + t;
                acc += csr_row_dot(aci, aval, arp[pos], arp[pos + 1], td);
            }
            gam += L[center] * acc;
        }
        qv[k] = acc;
    }
    __syncthreads();   // every wave is done reading the p image
#pragma unroll
    for (int k = 0; k < CG_MAXI; ++k) {
        const int it = wid + 4 * k;
        if (it >= nitems) continue;
        const int tyl = it / S2, t = it - tyl * S2;
        L[front + ((tyl + hy) * wx + lane + hx) * tpad + t] = qv[k];
    }
    __syncthreads();
    // 3. coalesced write-back of q (dim 2 fastest)
    const int nint = C.ty * CG_TX * S2;
    for (int j = threadIdx.x; j < nint; j += BLOCK) {
        const int r = (int)fdiv((uint32_t)j, C.fd_int);
        const int rem = j - r * (CG_TX * S2);
        const int xi = (int)fdiv((uint32_t)rem, C.fd_s2);
        const int t = rem - xi * S2;
        const int y = y0 + r, xx = x0 + xi;
        if (y < S0 && xx < S1) q[col0 + ((int64_t)y * S1 + xx) * S2 + t] = L[front + ((r + hy) * wx + xi + hx) * tpad + t];
    }
    store_partial(gam, part, blockIdx.x);
}

// Chunk mode: k_cg_normal on tiles that are also cut along dim 2 (cg_chunk_geometry), for grids whose
// whole dim-2 columns do not fit LDS (20 … 64 epochs).  A workgroup is one (tile, chunk), the chunks of
// a tile on consecutive ids (they share the lines of its columns).  Chunk ck owns t in
// [ck·S2/nch, (ck + 1)·S2/nch) and stages th more nodes on either side: image index
// front + (r·wx + xi)·tpad + (t − t0 + th).  Everything staged is z + β p_old — never the new p, which
// another workgroup may not have written yet — and only the owned (row, x, t) entries are written
// back as p, enter q and count in pᵀNp.  The partials leave through the same fixed-order sum as tile
// mode's, one slot per workgroup.
template <bool ATD = true>   // as k_cg_normal's
__global__ __launch_bounds__(BLOCK) void k_cg_normal_chunk(const CgState* __restrict__ st, const CgDesc* __restrict__ cd,
                                                           const double* __restrict__ coef, const double* __restrict__ z,
                                                           const double* __restrict__ pold, double* __restrict__ pnew,
                                                           double* __restrict__ q, const int32_t* __restrict__ arp,
                                                           const int32_t* __restrict__ aci,
                                                           const double* __restrict__ aval,
                                                           const double* __restrict__ td, double* __restrict__ part) {
    if (st->stop) return;
    const int tile = cg_tile_of_block();
    if (tile >= cd->ntiles) {
        if (threadIdx.x == 0) part[blockIdx.x] = 0.0;
        return;
    }
    int g = 0;
    while (g + 1 < cd->n_grids && tile >= cd->g[g + 1].tile0) ++g;   // tiles are numbered grid by grid
    const CgGrid& C = cd->g[g];
    const int tl = tile - C.tile0;
    const int tyx = tl / C.nch, ck = tl - tyx * C.nch;
    const int tyi = tyx / C.ntx;
    const int y0 = tyi * C.ty, x0 = (tyx - tyi * C.ntx) * CG_TX;
    const int S0 = C.shape[0], S1 = C.shape[1], S2 = C.shape[2];
    const int t0 = ck * S2 / C.nch, tlen = (ck + 1) * S2 / C.nch - t0;   // tc or tc − 1 nodes
    const int hy = C.hy, hx = C.hx, th = C.th, wx = C.wx, tpad = C.tpad, front = C.front;
    const int64_t col0 = C.col0;
    const double beta = st->beta;
    double* L = mf_zl;

    // 1. stage p = z + β p_old over the tile's rows, dim-1 positions and chunk, each with its halo;
    //    zeros outside the grid, in the padding of a column and in the front / back pads
    {
        const int rowlen = wx * tpad, img = (C.ty + 2 * hy) * rowlen, lds = C.lds, tw = tlen + 2 * th;
        for (int i0 = threadIdx.x; i0 < lds; i0 += CG_SU * BLOCK) {
            int64_t gi[CG_SU];
            bool ld[CG_SU], own[CG_SU];
#pragma unroll
            for (int k = 0; k < CG_SU; ++k) {
                const int i = i0 + k * BLOCK, ii = i - front;
                ld[k] = own[k] = false;
                gi[k] = 0;
                if (i < lds && ii >= 0 && ii < img) {
                    const int r = (int)fdiv((uint32_t)ii, C.fd_row);
                    const int rem = ii - r * rowlen;
                    const int xi = (int)fdiv((uint32_t)rem, C.fd_pad);
                    const int ti = rem - xi * tpad;
                    const int y = y0 - hy + r, x = x0 - hx + xi, t = t0 - th + ti;
                    if (ti < tw && t >= 0 && t < S2 && y >= 0 && y < S0 && x >= 0 && x < S1) {
                        ld[k] = true;
                        gi[k] = col0 + ((int64_t)y * S1 + x) * S2 + t;
                        own[k] = r >= hy && r < hy + C.ty && xi >= hx && xi < hx + CG_TX && ti >= th && ti < th + tlen;
                    }
                }
            }
            double zv[CG_SU], pv[CG_SU];
#pragma unroll
            for (int k = 0; k < CG_SU; ++k) {
                zv[k] = ld[k] ? z[gi[k]] : 0.0;
                pv[k] = ld[k] ? pold[gi[k]] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < CG_SU; ++k) {
                const int i = i0 + k * BLOCK;
                if (i < lds) {
                    const double v = zv[k] + beta * pv[k];
                    L[i] = v;
                    if (own[k]) pnew[gi[k]] = v;
                }
            }
        }
    }
    __syncthreads();

    // 2. q = N p + Adᵀt for the chunk's owned nodes, k_cg_normal's scheme: lane = dim-1 position, a
    //    wave takes (row, t) items wid, wid + 4, ...; the coefficient class of t is that of the
    //    absolute t; the coefficient row is wave-uniform when the tile is clear of both dim-1 edges
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nitems = C.ty * tlen;   // ≤ 4·CG_MAXI (cg_chunk_geometry)
    const int x = x0 + lane;
    const bool xin = x < S1;
    const int cx = cg_cls(xin ? x : 0, S1, C.K[1], C.ncls[1]);
    const bool xuni = x0 >= C.K[1] && x0 + CG_TX - 1 <= S1 - 1 - C.K[1];
    const int noff = C.noff;
    double qv[CG_MAXI];
    double gam = 0.0;
#pragma unroll
    for (int k = 0; k < CG_MAXI; ++k) {
        qv[k] = 0.0;
        const int it = wid + 4 * k;
        if (it >= nitems) continue;
        const int tyl = it / tlen, ti = it - tyl * tlen;
        const int y = y0 + tyl, t = t0 + ti;
        if (y >= S0) continue;
        const int cy = cg_cls(y, S0, C.K[0], C.ncls[0]), ct = cg_cls(t, S2, C.K[2], C.ncls[2]);
        const int center = front + ((tyl + hy) * wx + lane + hx) * tpad + ti + th;
        double acc = 0.0;
        if (xuni) {
            const int rb = __builtin_amdgcn_readfirstlane(C.coef0 + ((cy * C.ncls[1] + C.K[1]) * C.ncls[2] + ct) * noff);
            const double* __restrict__ cr = coef + rb;
            for (int o = 0; o < noff; ++o) acc += cr[o] * L[center + C.loff[o]];
        } else {
            const double* __restrict__ cr = coef + C.coef0 + ((cy * C.ncls[1] + cx) * C.ncls[2] + ct) * noff;
            for (int o = 0; o < noff; ++o) acc += cr[o] * L[center + C.loff[o]];
        }
        if (xin) {
            if (ATD) {
                const int64_t pos = (int64_t)C.node0 + ((int64_t)y * S1 + x) * S2 + t;
                acc += csr_row_dot(aci, aval, arp[pos], arp[pos + 1], td);
            }
            gam += L[center] * acc;
        }
        qv[k] = acc;
    }
    __syncthreads();   // every wave is done reading the p image
#pragma unroll
    for (int k = 0; k < CG_MAXI; ++k) {
        const int it = wid + 4 * k;
        if (it >= nitems) continue;
        const int tyl = it / tlen, ti = it - tyl * tlen;
        L[front + ((tyl + hy) * wx + lane + hx) * tpad + ti + th] = qv[k];
    }
    __syncthreads();
    // 3. coalesced write-back of q over the owned entries (dim 2 fastest)
    const int sel = tlen == C.tc ? 0 : 1;
    const int nint = C.ty * CG_TX * tlen;
    for (int j = threadIdx.x; j < nint; j += BLOCK) {
        const int r = (int)fdiv((uint32_t)j, C.fd_ic[sel]);
        const int rem = j - r * (CG_TX * tlen);
        const int xi = (int)fdiv((uint32_t)rem, C.fd_c[sel]);
        const int ti = rem - xi * tlen;
        const int y = y0 + r, xx = x0 + xi;
        if (y < S0 && xx < S1)
            q[col0 + ((int64_t)y * S1 + xx) * S2 + t0 + ti] = L[front + ((r + hy) * wx + xi + hx) * tpad + ti + th];
    }
    store_partial(gam, part, blockIdx.x);
}

// x (every CG_XK-th step, CgState::pend), s −= α q, z = M_b⁻¹ s = R_b⁻¹(R_b⁻ᵀ s) per column
// block, partial Σ sᵀz.  R_b⁻¹ is read as lf_t (bf16 by default, system.hpp; products in fp64):
// ~13 of the ~61 bytes per column the kernel moves.  The wave's consecutive blocks (one contiguous
// run) are copied to a wave-private LDS slice with coalesced loads, then each lane reads its row
// and column of R_b⁻¹ from LDS once per entry (lf_rowcol; in-order LDS per wave).
constexpr int BJ_NPK_MAX = BJ_LANES * (BJ_LANES + 1) / 2;
// 8-byte factor words one lane stages per wave step: the most over block sizes k ≤ K of
// (64/k blocks) × lf_stride(k(k+1)/2) entries (bf16, K = 12: 2; the generic bound 5 is fp32, k = 16)
constexpr int bj_words(int K) {
    int m = 1;
    for (int k = 1; k <= K; ++k) {
        const int npk = (k * (k + 1) / 2 + LF_PER8 - 1) / LF_PER8 * LF_PER8;
        const int w = ((64 / k) * npk / LF_PER8 + 63) / 64;
        m = w > m ? w : m;
    }
    return m;
}
template <bool AFF, int K, int NT = 0>   // K: loop length ≥ the block size (12 or BJ_LANES); NT: non-temporal bits
__global__ __launch_bounds__(BLOCK) void k_cg_block(const CgState* __restrict__ st, int64_t nb, int npks, BlkAffine aff,
                                                    int kaff, const int64_t* __restrict__ ptr,
                                                    const int32_t* __restrict__ cols,
                                                    const lf_t* __restrict__ Lf, CgP P,
                                                    const double* __restrict__ q, double* __restrict__ x,
                                                    double* __restrict__ s, double* __restrict__ z, double* part,
                                                    const uint8_t* __restrict__ live, const double* __restrict__ lam,
                                                    int dbg) {
    if (st->stop) return;
    // multigrid (lam: level 0's λ): z = c₂·M⁻¹s is the V-cycle's first Chebyshev step from x = 0
    // (k_mg_smooth, MG_XZERO: the same products, the same c₂), fused into this update
    double zs = 1.0;
    if (lam) {
        const double lmax = 1.1 * lam[0], lmin = 0.1 * lmax;
        zs = 1.0 / (0.5 * (lmax + lmin));
    }
    constexpr int NV = bj_words(K);
    __shared__ double LR[BLOCK / 64][NV * 64];           // ≤ 64/k blocks × npks factor entries per wave
    const bool xupd = st->pend == CG_XK - 1;   // this step pays the three owed α p and its own α_k p_k
    const double a0 = st->pend_a[0], a1 = st->pend_a[1], a2 = st->pend_a[2];
    __shared__ double SX[BLOCK / 64][64 + BJ_LANES];    // s then w of the wave's lanes (exchange)
    const double alpha = st->alpha;
    // L lanes per block, W blocks per wave and step: affine blocks use exactly k lanes (C4: 5
    // blocks of 12 per wave, 94 % of the lanes busy), general blocks 16
    const int lane = threadIdx.x & 63;
    const int L = AFF ? kaff : BJ_LANES, W = 64 / L;
    const int grp = AFF ? lane / L : lane >> 4, j = lane - grp * L, gbase = grp * L;
    double* R4 = LR[threadIdx.x >> 6];
    if (lane < BJ_LANES) SX[threadIdx.x >> 6][64 + lane] = 0.0;   // read (× 0) by the last group
    const int64_t wstride = (int64_t)gridDim.x * (BLOCK / 64) * W;
    // this lane's affine column (base_j, stride_j), read once: indexing the by-value argument
    // arrays with a lane-varying j inside the loop costs a scalar loop per step
    int64_t abase = 0, astride = 0;
    if (AFF) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (i == j) {
                abase = aff.base[i];
                astride = aff.stride[i];
            }
    }
    // one wave step's operands: its blocks' q, s (and x, the four owed p on x steps) and the
    // factor words it stages
    struct Ops {
        double q, s, x, p0, p1, p2, p3, v[NV];
    };
    auto column = [&](int64_t b0, int& k, int64_t& c) {
        const int64_t b = b0 + grp;
        const bool have = grp < W && b < nb;
        if (AFF) {   // column ids from the affine block structure: no index loads
            k = have ? kaff : 0;
            c = j < k ? abase + b * astride : 0;
        } else {
            const int64_t e0 = have ? ptr[b] : 0;
            k = have ? (int)(ptr[b + 1] - e0) : 0;
            c = j < k ? cols[e0 + j] : 0;
        }
        return j < k && (!live || live[c]);   // distributed ranks: owned columns only
    };
    auto fetch = [&](int64_t b0, Ops& o) {
        int k;
        int64_t c;
        const bool mine = column(b0, k, c), mx = mine && xupd;
        o.q = mine ? q[c] : 0.0;
        o.s = mine ? s[c] : 0.0;
        o.x = mx ? x[c] : 0.0;
        o.p0 = mx ? P.p[0][c] : 0.0;
        o.p1 = mx ? P.p[1][c] : 0.0;
        o.p2 = mx ? P.p[2][c] : 0.0;
        o.p3 = mx ? P.p[3][c] : 0.0;
        const int cnt = (int)(min<int64_t>(W, nb - b0) * npks / LF_PER8);   // 8-byte words
        const double* __restrict__ src = reinterpret_cast<const double*>(Lf + b0 * npks);
#pragma unroll
        for (int i = 0; i < NV; ++i)
            o.v[i] = lane + 64 * i < cnt ? ((NT & 1) ? __builtin_nontemporal_load(src + lane + 64 * i) : src[lane + 64 * i])
                                         : 0.0;
    };
    double sr = 0.0;
    auto step = [&](int64_t b0, const Ops& o) {
        int k;
        int64_t c;
        const bool mine = column(b0, k, c);
        const int cnt = (int)(min<int64_t>(W, nb - b0) * npks / LF_PER8);
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (lane + 64 * i < cnt) R4[lane + 64 * i] = o.v[i];
        const double sn = o.s - alpha * o.q;
        const double xn = (((o.x + a0 * o.p0) + a1 * o.p1) + a2 * o.p2) + alpha * o.p3;
        if (dbg & 1) {   // LSQ_CG_BLOCK_DBG bit 0 (development, results wrong): z = s, no block products
            if (mine) {
                if (xupd) x[c] = xn;
                s[c] = sn;
                z[c] = sn + R4[lane] * 1e-300;
                sr += sn * sn;
            }
            return;
        }
        const lf_t* M = reinterpret_cast<const lf_t*>(R4) + grp * npks;
        // the block's values reach its lanes through the wave's LDS row (LDS runs a wave's
        // operations in order): one write and k/2 paired reads instead of 2k cross-lane shuffles
        double* X = SX[threadIdx.x >> 6];
        const double* Xb = X + gbase;
        double w = 0.0, zz = 0.0;
        if (NT & 8) {   // column and row of R_b⁻¹ read separately (2k LDS reads; round-5 closing form)
            float lcol[K], lrow[K];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                lcol[i] = (mine && i <= j) ? lf_val(M[j * (j + 1) / 2 + i]) : 0.0f;
                lrow[i] = (mine && i >= j && i < k) ? lf_val(M[i * (i + 1) / 2 + j]) : 0.0f;
            }
            X[lane] = sn;
#pragma unroll
            for (int i = 0; i < K; ++i) w += (double)lcol[i] * Xb[i];
            X[lane] = w;
#pragma unroll
            for (int i = 0; i < K; ++i) zz += (double)lrow[i] * Xb[i];
        } else {
            float fv[K];   // column j and row j of R_b⁻¹ (this lane plays j), one read per entry
            lf_rowcol<K>(M, j, k, mine, fv);
            X[lane] = sn;
            // w = R_b⁻ᵀ s: w_j = Σ_{i≤j} (R_b⁻¹)_ij s_i
#pragma unroll
            for (int i = 0; i < K; ++i) w += (i <= j ? (double)fv[i] : 0.0) * Xb[i];
            X[lane] = w;
            // z = R_b⁻¹ w: z_j = Σ_{i≥j} (R_b⁻¹)_ji w_i
#pragma unroll
            for (int i = 0; i < K; ++i) zz += (i >= j ? (double)fv[i] : 0.0) * Xb[i];
        }
        if (mine) {
            const double zn = lam ? zs * zz : zz;
            if (xupd) {
                if (NT & 2) __builtin_nontemporal_store(xn, x + c);
                else x[c] = xn;
            }
            if (NT & 4) {
                __builtin_nontemporal_store(sn, s + c);
                __builtin_nontemporal_store(zn, z + c);
            } else {
                s[c] = sn;
                z[c] = zn;
            }
            sr += sn * zz;
        }
    };
    // one wave step at a time: loading the next step's operands ahead of this step's block
    // products (held in registers) measured no faster (C4: 173–175 µs either way, round 5)
    for (int64_t b0 = ((int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6)) * W; b0 < nb; b0 += wstride) {
        Ops o;
        fetch(b0, o);
        step(b0, o);
    }
    store_partial(sr, part, blockIdx.x);
}

// Jacobi variant over the full space: z = s / ‖A_j‖² (csf = 1/‖A_j‖, 0 = removed column)
__global__ __launch_bounds__(BLOCK) void k_cg_jacobi(const CgState* __restrict__ st, int64_t nf,
                                                     const double* __restrict__ csf, CgP P,
                                                     const double* __restrict__ q, double* __restrict__ x,
                                                     double* __restrict__ s, double* __restrict__ z, double* part) {
    if (st->stop) return;
    const double alpha = st->alpha;
    const bool xupd = st->pend == CG_XK - 1;   // x every CG_XK-th step, as k_cg_block
    const double a0 = st->pend_a[0], a1 = st->pend_a[1], a2 = st->pend_a[2];
    double sr = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < nf; j += (int64_t)gridDim.x * BLOCK) {
        const double c = csf[j];
        if (c == 0.0) continue;
        if (xupd) x[j] = (((x[j] + a0 * P.p[0][j]) + a1 * P.p[1][j]) + a2 * P.p[2][j]) + alpha * P.p[3][j];
        const double sn = s[j] - alpha * q[j];
        const double zz = (c * c) * sn;
        s[j] = sn;
        z[j] = zz;
        sr += sn * zz;
    }
    store_partial(sr, part, blockIdx.x);
}

// the owed α p of a solve that stopped inside an x cycle (phases 0 … pend − 1; full space; p = 0 off
// the kept columns)
__global__ __launch_bounds__(BLOCK) void k_cg_xfix(const CgState* __restrict__ st, int64_t nf, CgP P,
                                                   double* __restrict__ x) {
    const int c = st->pend;
    if (!c) return;
    const double a0 = st->pend_a[0], a1 = st->pend_a[1], a2 = st->pend_a[2];
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < nf; j += (int64_t)gridDim.x * BLOCK) {
        double v = x[j] + a0 * P.p[0][j];
        if (c > 1) v += a1 * P.p[1][j];
        if (c > 2) v += a2 * P.p[2][j];
        x[j] = v;
    }
}

// init: ‖r0‖² = Σu², ‖b‖ = sqrt(Σ(w∘b)²) from the LSQR init partials
// gs (distributed ranks): all-reduced sums instead of the partials — [0] Σu², [3] Σ(w∘b)²
__global__ __launch_bounds__(BLOCK) void k_cg_init(CgState* st, const double* part_u, int nu, const double* part_b,
                                                   int nbp, const double* gs) {
    const double su = gs ? gs[0] : reduce_parts(part_u, nu);
    const double sb = gs ? gs[3] : reduce_parts(part_b, nbp);
    if (threadIdx.x) return;
    st->rn2 = su;
    st->bnorm = sqrt(sb);
    st->alpha = 0.0;
    st->beta = 0.0;
}

// gsum (distributed ranks): [4] + [5] all-reduced instead of the partials
__device__ __forceinline__ void cg_alpha_body(CgState* st, const double* part_g, int ng, const double* part_t, int nt,
                                              const double* gsum);
__global__ __launch_bounds__(BLOCK) void k_cg_alpha(CgState* st, const double* part_g, int ng, const double* part_t,
                                                    int nt, const double* gsum) {
    cg_alpha_body(st, part_g, ng, part_t, nt, gsum);
}
// α_k = ρ_k / pᵀNp from the operator's partials (every thread of one workgroup calls it)
__device__ __forceinline__ void cg_alpha_body(CgState* st, const double* part_g, int ng, const double* part_t, int nt,
                                              const double* gsum) {
    if (st->stop) return;
    const double gs = gsum ? gsum[4] : reduce_parts(part_g, ng);
    const double gt = gsum ? gsum[5] : nt ? reduce_parts(part_t, nt) : 0.0;   // column mode: pᵀN_s p + ‖Ad p‖²
    const double gam = gs + gt;
    if (threadIdx.x) return;
    st->gamma = gam;
    if (!(gam > 0.0)) {   // p = 0: the previous iterate is exact
        st->stop = 1;
        st->istop = 1;
        st->alpha = 0.0;
        return;
    }
    const double a = st->rho / gam, b = st->beta;   // α_k, β_{k−1}
    // Lanczos tridiagonal T = BᵀB of the equivalent LSQR bidiagonalisation: T_kk = 1/α_k + β_{k−1}/α_{k−1},
    // and LSQR's ‖A‖ estimate is sqrt(trace T) = sqrt(Σ α_i² + β_{i+1}²)
    st->anorm2 += 1.0 / a + (st->itn > 0 ? b / st->alpha_prev : 0.0);
    // ‖Δy‖² of the correction in preconditioned coordinates: p̃_k ⊥ s̃_{k+1}, so
    // ‖p̃_k‖² = ρ_k + β²‖p̃_{k−1}‖², Δy_kᵀp̃_k = β(Δy_{k−1}ᵀp̃_{k−1} + α_{k−1}‖p̃_{k−1}‖²)
    const double pn = st->rho + b * b * st->pn2;
    const double dp = b * (st->dp + st->alpha_prev * st->pn2);
    st->dn2 += 2.0 * a * dp + a * a * pn;
    st->pn2 = pn;
    st->dp = dp;
    st->alpha_prev = a;
    st->alpha = a;
}

// mode 1: init (ρ0); mode 0: iteration
// gsum (distributed ranks): [6] all-reduced instead of the partials
__global__ __launch_bounds__(BLOCK) void k_cg_beta(CgState* st, const double* part_r, int nr, int mode,
                                                   const double* gsum) {
    if (mode == 0 && st->stop) return;
    const double rho_new = gsum ? gsum[6] : reduce_parts(part_r, nr);
    if (threadIdx.x) return;
    const double eps = 2.220446049250313e-16;
    if (mode == 1) {
        st->rho = rho_new;
        st->beta = 0.0;
        st->itn = 0;
        st->r1norm = sqrt(st->rn2);
        st->arnorm = sqrt(rho_new);
        if (!(rho_new > 0.0) || !(st->bnorm > 0.0)) {   // Aᵀr0 = 0: x0 is the solution
            st->stop = 1;
            st->istop = 0;
        }
        return;
    }
    if (st->pend == CG_XK - 1) {   // the update kernel paid the cycle's owed steps and its own
        st->pend = 0;
    } else {                       // it skipped x: α_k p_k is owed to the cycle's last step (or to k_cg_xfix)
        st->pend_a[st->pend] = st->alpha;
        st->pend += 1;
    }
    st->rn2 = fmax(st->rn2 - st->alpha * st->rho, 0.0);
    st->beta = rho_new / st->rho;
    st->rho = rho_new;
    st->itn += 1;
    const double anorm = fmax(sqrt(st->anorm2), st->anorm_seed), rnorm = sqrt(st->rn2), xnorm = sqrt(st->dn2), bnorm = st->bnorm;
    const double arnorm = sqrt(rho_new);
    st->anorm = anorm;
    st->r1norm = rnorm;
    st->arnorm = arnorm;
    st->xnorm = xnorm;
    const double test1 = rnorm / bnorm;
    const double test2 = arnorm / (anorm * rnorm + eps);
    const double t1 = test1 / (1.0 + anorm * xnorm / bnorm);
    const double rtol = st->btol + st->atol * anorm * xnorm / bnorm;
    int istop = 0;
    if (st->itn >= st->maxit) istop = 7;
    if (!st->no_stop) {
        if (1.0 + test2 <= 1.0) istop = 5;
        if (1.0 + t1 <= 1.0) istop = 4;
        if (test2 <= st->atol) istop = 2;
        if (test1 <= rtol) istop = 1;
    }
    st->istop = istop;
    if (istop) st->stop = 1;
}

__global__ __launch_bounds__(BLOCK) void k_cg_scatter(int64_t n, const int32_t* __restrict__ keep,
                                                      const double* __restrict__ xc, double* __restrict__ xf) {
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * BLOCK)
        xf[keep[j]] = xc[j];
}

__global__ __launch_bounds__(BLOCK) void k_cg_gather(int64_t n, const int32_t* __restrict__ keep,
                                                     const double* __restrict__ xf, double* __restrict__ xc) {
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * BLOCK)
        xc[j] = xf[keep[j]];
}

__global__ __launch_bounds__(BLOCK) void k_count_nonempty(int64_t rows, const int32_t* __restrict__ rp,
                                                          unsigned long long* out) {
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < rows; i += (int64_t)gridDim.x * BLOCK)
        c += rp[i + 1] > rp[i] ? 1ull : 0ull;
    c = (unsigned long long)wave_sum((double)c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

// Field-valued parts of a 2-D grid (system.hpp CgVar; the anisotropic notebook's directional
// operator A_v, whose rows are scaled by a direction field, so AᵀA is not a class-table stencil).
// One workgroup per tile of CGV_TY × CGV_TX nodes:
//   t_c  = w Σ_e a_e(c) p[c + o_e]           at the centres of the tile and its R-halo (a_e = val_e·F),
//   q_i += w Σ_e a_e(i − o_e) t_{i − o_e}    at the tile's nodes,
//   Σ t_c² over the tile's own centres       (= pᵀA_vᵀA_v p: every row lives in one tile).
// p (2R halo), the fields and t of the centre region are staged in LDS; a centre outside the
// part's box has fields 0, so it contributes nothing.  Runs after the normal kernel has written p
// and q (RMW of q at the grid's nodes: same stream as the x-edge pass, before Adᵀt).
template <int R>
__global__ __launch_bounds__(BLOCK) void k_cg_var2d(const CgState* __restrict__ st, CgVar V,
                                                    const double* __restrict__ p, double* __restrict__ q,
                                                    double* __restrict__ part) {
    extern __shared__ double cgv_lds[];
    constexpr int TY = CGV_TY, TX = CGV_TX, PH = TY + 4 * R, PW = TX + 4 * R, CH = TY + 2 * R, CW = TX + 2 * R;
    constexpr int NC = CH * CW;
    if (st && st->stop) return;
    double* Pl = cgv_lds;
    double* Tl = Pl + PH * PW;
    double* Fl = Tl + NC;
    const int b = blockIdx.x;
    const int ty = b / V.ntx, tx = b - ty * V.ntx;
    const int y0 = ty * TY, x0 = tx * TX;
    for (int i = threadIdx.x; i < PH * PW; i += BLOCK) {
        const int ry = i / PW, rx = i - ry * PW;
        const int y = y0 - 2 * R + ry, x = x0 - 2 * R + rx;
        Pl[i] = (y >= 0 && y < V.S0 && x >= 0 && x < V.S1) ? p[(int64_t)V.col0 + (int64_t)y * V.S1 + x] : 0.0;
    }
    const int W1 = V.hi1 - V.lo1;
    for (int i = threadIdx.x; i < NC; i += BLOCK) {
        const int cy = i / CW, cx = i - cy * CW;
        const int y = y0 - R + cy, x = x0 - R + cx;
        const bool in = y >= V.lo0 && y < V.hi0 && x >= V.lo1 && x < V.hi1;
        const int64_t k = in ? (int64_t)(y - V.lo0) * W1 + (x - V.lo1) : 0;
        for (int f = 0; f < V.nfield; ++f) Fl[f * NC + i] = in ? V.F[f * V.n_eq + k] : 0.0;
    }
    __syncthreads();
    double acc = 0.0;
    for (int i = threadIdx.x; i < NC; i += BLOCK) {
        const int cy = i / CW, cx = i - cy * CW;
        double t = 0.0;
        for (int e = 0; e < V.ntpl; ++e)
            t += (V.val[e] * Fl[V.fsel[e] * NC + i]) * Pl[(cy + R + V.oy[e]) * PW + (cx + R + V.ox[e])];
        t *= V.w;
        Tl[i] = t;
        if (cy >= R && cy < R + TY && cx >= R && cx < R + TX) acc += t * t;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TY * TX; i += BLOCK) {
        const int iy = i / TX, ix = i - iy * TX;
        const int y = y0 + iy, x = x0 + ix;
        if (y >= V.S0 || x >= V.S1) continue;
        double s = 0.0;
        for (int e = 0; e < V.ntpl; ++e) {
            const int c = (iy + R - V.oy[e]) * CW + (ix + R - V.ox[e]);
            s += (V.val[e] * Fl[V.fsel[e] * NC + c]) * Tl[c];
        }
        const int64_t gi = (int64_t)V.col0 + (int64_t)y * V.S1 + x;
        q[gi] += V.w * s;
    }
    store_partial(acc, part, V.blk0 + b);
}

size_t cg_var_lds(const CgVar& V) {
    const int R = V.R, NC = (CGV_TY + 2 * R) * (CGV_TX + 2 * R);
    return sizeof(double) * ((size_t)(CGV_TY + 4 * R) * (CGV_TX + 4 * R) + (size_t)NC * (1 + V.nfield));
}

// Stencil parts with a row scale per (y, x) node on 2-D and 3-D grids (system.hpp CgSc; lsq_set_cg_scaled:
// the constraint rows of a masked fit or of constraint_scaling_maps), k_cg_var2d's counterpart.  One
// workgroup per tile of G.ty × CGS_TX nodes × the whole dim-2 column; for each scaled part of the grid
//   t_c  = W2(c) Σ_e v_e p[c + o_e]          at the centres of the tile and its R halo (0 outside the box),
//   q_i += Σ_e v_e t_{i − o_e}               at the tile's nodes (summed over the parts in registers),
//   Σ W2 (Σ_e v_e p)²                        over the tile's own centres (every row lives in one tile).
// p (2R halo) and t are staged in LDS with the odd dim-2 stride G.sp.  The columns of a node are
// contiguous in t, then x: an image row is one contiguous run of global memory, and lanes walk it in
// that order in the staging loop and in the q update.  The part loop and every sum run in a fixed
// order, no atomics.  A removed column (the reference epoch) holds p = 0 like everywhere in the step,
// and its q is never read.  Same stream and place as k_cg_var2d: RMW of q behind the normal kernel and
// the x-edge pass, before the node gather.
__global__ __launch_bounds__(BLOCK) void k_cg_scaled(const CgState* __restrict__ st, CgSc G,
                                                     const CgScPart* __restrict__ parts,
                                                     const double* __restrict__ W2, const double* __restrict__ p,
                                                     double* __restrict__ q, double* __restrict__ part) {
    extern __shared__ double cgs_lds[];
    if (st && st->stop) return;
    const int R = G.R, TY = G.ty, SP = G.sp, S2 = G.S2;
    const int PH = TY + 4 * R, PW = CGS_TX + 4 * R, CH = TY + 2 * R, CW = CGS_TX + 2 * R;
    double* Pl = cgs_lds;
    double* Tl = Pl + PH * PW * SP;
    const int b = blockIdx.x;
    const int ty = b / G.ntx, tx = b - ty * G.ntx;
    const int y0 = ty * TY, x0 = tx * CGS_TX;
    const uint32_t rowlen = (uint32_t)(PW * S2);
    for (uint32_t i = threadIdx.x; i < (uint32_t)PH * rowlen; i += BLOCK) {
        const uint32_t ry = i / rowlen, j = i - ry * rowlen;
        const uint32_t rx = fdiv(j, G.fd_s2), t = j - rx * (uint32_t)S2;
        const int y = y0 - 2 * R + (int)ry, x = x0 - 2 * R + (int)rx;
        Pl[(ry * PW + rx) * SP + t] =
            (y >= 0 && y < G.S0 && x >= 0 && x < G.S1) ? p[(int64_t)G.col0 + ((int64_t)y * G.S1 + x) * S2 + t] : 0.0;
    }
    const int nn = TY * CGS_TX * S2;   // ≤ CGS_ITEMS · BLOCK (cg_describe)
    double qa[CGS_ITEMS];
#pragma unroll
    for (int k = 0; k < CGS_ITEMS; ++k) qa[k] = 0.0;
    double acc = 0.0;
    for (int qq = 0; qq < G.np; ++qq) {
        const CgScPart& P = parts[G.part0 + qq];
        const int W1 = P.hi[1] - P.lo[1];
        __syncthreads();   // p staged; the previous part's t read
        for (uint32_t i = threadIdx.x; i < (uint32_t)(CH * CW * S2); i += BLOCK) {
            const uint32_t cc = fdiv(i, G.fd_s2), t = i - cc * (uint32_t)S2;
            const int cy = (int)(cc / (uint32_t)CW), cx = (int)cc - cy * CW;
            const int y = y0 - R + cy, x = x0 - R + cx;
            double tv = 0.0;
            if (y >= P.lo[0] && y < P.hi[0] && x >= P.lo[1] && x < P.hi[1] && (int)t >= P.lo[2] && (int)t < P.hi[2]) {
                double s = 0.0;   // every entry of an existing row lies inside the grid (cg_describe checks it)
                for (int e = 0; e < P.ntpl; ++e)
                    s += P.val[e] * Pl[((cy + R + P.oy[e]) * PW + (cx + R + P.ox[e])) * SP + (int)t + P.ot[e]];
                tv = W2[P.w2 + (int64_t)(y - P.lo[0]) * W1 + (x - P.lo[1])] * s;
                if (cy >= R && cy < R + TY && cx >= R && cx < R + CGS_TX) acc += tv * s;
            }
            Tl[cc * SP + t] = tv;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CGS_ITEMS; ++k) {
            const int i = (int)threadIdx.x + k * BLOCK;
            if (i >= nn) continue;
            const uint32_t nd = fdiv((uint32_t)i, G.fd_s2);
            const int t = i - (int)nd * S2, iy = (int)(nd / CGS_TX), ix = (int)(nd % CGS_TX);
            double s = 0.0;
            for (int e = 0; e < P.ntpl; ++e) {
                const int tt = t - P.ot[e];
                if (tt >= 0 && tt < S2)
                    s += P.val[e] * Tl[((iy + R - P.oy[e]) * CW + (ix + R - P.ox[e])) * SP + tt];
            }
            qa[k] += s;
        }
    }
#pragma unroll
    for (int k = 0; k < CGS_ITEMS; ++k) {
        const int i = (int)threadIdx.x + k * BLOCK;
        if (i >= nn) continue;
        const uint32_t nd = fdiv((uint32_t)i, G.fd_s2);
        const int t = i - (int)nd * S2, y = y0 + (int)(nd / CGS_TX), x = x0 + (int)(nd % CGS_TX);
        if (y < G.S0 && x < G.S1) q[(int64_t)G.col0 + ((int64_t)y * G.S1 + x) * S2 + t] += qa[k];
    }
    store_partial(acc, part, G.blk0 + b);
}

inline size_t cg_sc_lds(const CgSc& G) {
    return sizeof(double) * (size_t)G.sp *
           ((size_t)(G.ty + 4 * G.R) * (CGS_TX + 4 * G.R) + (size_t)(G.ty + 2 * G.R) * (CGS_TX + 2 * G.R));
}

// A scaled part's field W2 = rs² over its (y, x) centre box from the row scales (weight × row mask) of
// its rows at dim-2 position lo2; bad[0] = 1 when some (y, x) holds two scales that differ in a bit
__global__ __launch_bounds__(BLOCK) void k_cg_sc_field(int32_t row0, int32_t n0, int32_t n1, int32_t n2, int32_t bs0,
                                                       int32_t bs1, int32_t bs2, const double* __restrict__ rs,
                                                       double* __restrict__ W2, int32_t* __restrict__ bad) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < (int64_t)n0 * n1; i += (int64_t)gridDim.x * BLOCK) {
        const int64_t yy = i / n1, xx = i - yy * n1;
        const int64_t r = (int64_t)row0 + yy * bs0 + xx * bs1;
        const double w = rs[r];
        bool same = true;
        for (int k = 1; k < n2; ++k) same = same && __double_as_longlong(rs[r + (int64_t)k * bs2]) == __double_as_longlong(w);
        if (!same) bad[0] = 1;
        W2[i] = w * w;
    }
}

// q += A_vᵀA_v p for every field-valued part (partials at part + V.blk0), then q += A_qᵀ W2 A_q p for
// every part with a row scale per (y, x) node, a launch per grid (partials at part + G.blk0)
struct CgMarks;
void cg_mark_scaled(CgMarks* m, hipStream_t st);   // the profilers' mark in front of k_cg_scaled (CG_SCALED0)
void cg_launch_var(const System& S, const double* p, double* q, double* part, hipStream_t st, const CgState* cst,
                   CgMarks* marks = nullptr) {
    for (const CgVar& V : S.cg_var) {
        const dim3 grid((unsigned)(V.nty * V.ntx));
        if (V.R == 1)
            hipLaunchKernelGGL(k_cg_var2d<1>, grid, dim3(BLOCK), cg_var_lds(V), st, cst, V, p, q, part);
        else
            hipLaunchKernelGGL(k_cg_var2d<2>, grid, dim3(BLOCK), cg_var_lds(V), st, cst, V, p, q, part);
    }
    if (marks && !S.cg_sc.empty()) cg_mark_scaled(marks, st);
    for (const CgSc& G : S.cg_sc)
        hipLaunchKernelGGL(k_cg_scaled, dim3((unsigned)(G.nty * G.ntx)), dim3(BLOCK), cg_sc_lds(G), st, cst, G,
                           S.cg_scp.p, S.cg_scw.p, p, q, part);
}

// ---- host: normal-stencil description ------------------------------------------------------

int cls_rep(int k, int n, int K, int ncls) { return ncls == n ? k : (k <= K ? k : n - 2 * K - 1 + k); }
int cls_of(int c, int n, int K, int ncls) { return ncls == n ? c : (c < K ? c : (c >= n - K ? c - n + 2 * K + 1 : K)); }

// The normal stencil of grid g's stencil parts as a class table (tile layout, t by class):
//   (AᵀA)_{c, c+d} = Σ_q w_q² Σ_{t1,t2: o_t2 − o_t1 = d} v_t1 v_t2 · [c − o_t1 ∈ box_q]
// evaluated at the representative node of each boundary class.  T.on = false for a grid without
// parts.  False (+ reason) when the structured normal operator does not apply.
// scaled (lsq_set_cg_scaled): a part with per-row scales is left out of the table, as a field-valued one
// is (k_cg_scaled applies it; cg_describe checks that its scales are one per (y, x) node).
bool ns_from_parts(const MfDesc& d, int g, NsTable& T, std::string& why, bool scaled = false) {
    const MfGrid& G = d.g[g];
    T = NsTable{};
    for (int e = 0; e < 3; ++e) T.shape[e] = G.shape[e];
    T.col0 = G.col0;
    T.node0 = G.node0;
    if (!G.nparts) return true;
    T.on = true;
    std::vector<std::array<int, 3>>& offs = T.offs;
    int K[3] = {0, 0, 0};
    for (int qq = 0; qq < G.nparts; ++qq) {
        const MfPart& P = d.p[G.part[qq]];
        if (!P.wconst && (!scaled || P.var)) {
            why = "a stencil part has per-row scales (masked or non-uniform constraint rows)";
            return false;
        }
        if (P.var || !P.wconst) continue;   // field-valued: k_cg_var2d; scaled: k_cg_scaled
        for (int e = 0; e < 3; ++e) {
            int omin = 1 << 20, omax = -(1 << 20);
            for (int t = 0; t < P.ntpl; ++t) {
                omin = std::min(omin, P.off[t][e]);
                omax = std::max(omax, P.off[t][e]);
            }
            K[e] = std::max({K[e], P.lo[e] + omax, G.shape[e] - P.hi[e] - omin, 0});
        }
        for (int t1 = 0; t1 < P.ntpl; ++t1)
            for (int t2 = 0; t2 < P.ntpl; ++t2) {
                const std::array<int, 3> dd = {P.off[t2][0] - P.off[t1][0], P.off[t2][1] - P.off[t1][1],
                                               P.off[t2][2] - P.off[t1][2]};
                if (std::find(offs.begin(), offs.end(), dd) == offs.end()) offs.push_back(dd);
            }
    }
    if (offs.empty()) offs.push_back({0, 0, 0});   // only field-valued or scaled parts: a zero class table
    if ((int)offs.size() > CG_MAX_OFF) { why = "normal stencil wider than CG_MAX_OFF"; return false; }
    std::sort(offs.begin(), offs.end());
    for (int e = 0; e < 3; ++e) {
        T.K[e] = K[e];
        T.ncls[e] = G.shape[e] <= 2 * K[e] + 1 ? G.shape[e] : 2 * K[e] + 1;
    }
    const int noff = (int)offs.size();
    T.coef.assign((size_t)T.ncls[0] * T.ncls[1] * T.ncls[2] * noff, 0.0);
    for (int cy = 0; cy < T.ncls[0]; ++cy)
        for (int cx = 0; cx < T.ncls[1]; ++cx)
            for (int ct = 0; ct < T.ncls[2]; ++ct) {
                const int pos[3] = {cls_rep(cy, G.shape[0], K[0], T.ncls[0]), cls_rep(cx, G.shape[1], K[1], T.ncls[1]),
                                    cls_rep(ct, G.shape[2], K[2], T.ncls[2])};
                double* row = T.coef.data() + ((size_t)(cy * T.ncls[1] + cx) * T.ncls[2] + ct) * noff;
                for (int qq = 0; qq < G.nparts; ++qq) {
                    const MfPart& P = d.p[G.part[qq]];
                    if (P.var || !P.wconst) continue;
                    for (int t1 = 0; t1 < P.ntpl; ++t1) {
                        bool in = true;   // the row centred at pos − o_t1 exists
                        for (int e = 0; e < 3; ++e) {
                            const int ce = pos[e] - P.off[t1][e];
                            in = in && ce >= P.lo[e] && ce < P.hi[e];
                        }
                        if (!in) continue;
                        for (int t2 = 0; t2 < P.ntpl; ++t2) {
                            const std::array<int, 3> dd = {P.off[t2][0] - P.off[t1][0], P.off[t2][1] - P.off[t1][1],
                                                           P.off[t2][2] - P.off[t1][2]};
                            const int o = (int)(std::find(offs.begin(), offs.end(), dd) - offs.begin());
                            row[o] += (P.w * P.val[t1]) * (P.w * P.val[t2]);
                        }
                    }
                }
            }
    return true;
}

// Device description of the normal operator over grids T[0 .. n_grids) (grids with T.on carry a
// stencil): strip / tile geometry, column-mode groups, and the two coefficient tables
//   tile mode:   coef [coef0 + ((cy·ncls1 + cx)·ncls2 + ct)·noff + o]
//   column mode: coefc[coefc0 + (cy·ncls1 + cx)·rowlen + gc[grp] + t·(2DT+1) + dt + DT]  (exact t)
// The column-mode rows are read from the tile table at t's class (the same sums, bit for bit).
static inline int offs_of(const NsTable& N, int o, int e) { return N.offs[o][e]; }

// Chunk mode's geometry of a grid whose tile-mode image exceeds LDS: tiles of ty rows × CG_TX dim-1
// positions × one chunk of dim 2, a chunk being ≤ tc owned nodes with ht halo nodes on either side in
// a column of odd stride tpad ≥ tc + 2·ht.  Both caps hold: the image (with its pads) within 64 KB and
// ty·tc ≤ 4·CG_MAXI items.
//   1. (ty*, tc*) = the pair with the smallest staged-to-owned ratio (ty + 2hy)(tc + 2ht) / (ty·tc)
//      (the factor wx / CG_TX is common); ties: more items, then the longer chunk (longer runs along
//      the fastest dimension).  hy = hx = ht = 2: (5, 9), 9·68·13 = 7 956 doubles, ratio 2.76.
//   2. dim 2 is cut into nch = ceil(S2 / tc*) chunks of near-equal length, chunk k owning
//      [k·S2/nch, (k + 1)·S2/nch): tc = ceil(S2 / nch) ≤ tc*.
//   3. ty = the most rows ≤ S0 both caps admit at that tc (the ratio falls with ty): 20 and 28 epochs
//      run chunks of 7 in an 11-stride image with 6 rows (2.78 instead of (5, 7)'s 3.01).
// False when no pair fits.
static bool cg_chunk_geometry(CgGrid& C) {
    const int S2 = C.shape[2], hy = C.hy, ht = C.ht, cap = 64 * 1024 / (int)sizeof(double);
    auto pad = [&](int tc) { return (tc + 2 * ht) | 1; };
    auto fits = [&](int ty, int tc) {
        return ty * tc <= 4 * CG_MAXI && C.front + (ty + 2 * hy) * C.wx * pad(tc) + ht <= cap;
    };
    int by = 0, bc = 0;
    for (int ty = 1; ty <= 4 * CG_MAXI; ++ty)
        for (int tc = 1; tc <= std::min(S2, 4 * CG_MAXI / ty); ++tc) {
            if (!fits(ty, tc)) continue;
            const int64_t n = (int64_t)(ty + 2 * hy) * (tc + 2 * ht), d = ty * tc;
            const int64_t bn = (int64_t)(by + 2 * hy) * (bc + 2 * ht), bd = by * bc;
            if (!by || n * bd < bn * d || (n * bd == bn * d && (d > bd || (d == bd && tc > bc)))) {
                by = ty;
                bc = tc;
            }
        }
    if (!by) return false;
    C.nch = (S2 + bc - 1) / bc;
    C.tc = (S2 + C.nch - 1) / C.nch;
    int ty = std::min(by, C.shape[0]);
    while (ty < C.shape[0] && fits(ty + 1, C.tc)) ++ty;
    C.ty = ty;
    C.th = ht;
    C.tpad = pad(C.tc);
    C.lds = C.front + (ty + 2 * hy) * C.wx * C.tpad + ht;
    for (int o = 0; o < C.noff; ++o) C.loff[o] = (C.ooff[o][0] * C.wx + C.ooff[o][1]) * C.tpad + C.ooff[o][2];
    return true;
}

// chunks (cg_describe alone passes it, from lsq_set_cg_chunks): a grid of ≤ 4·CG_MAXI nodes along dim
// 2 whose tile-mode image exceeds 64 KB of LDS is cut along dim 2 too (cg_chunk_geometry) instead of
// being refused, and the description is chunk mode's (c.chunk; colmode 0: tile mode's step).  Layouts
// that are column or tile mode without the flag are the same with it.
bool cg_layout(const std::vector<NsTable>& T, int cus, CgDesc& c, std::vector<double>& coef,
               std::vector<double>& coefc, std::string& why, bool chunks = false) {
    c = CgDesc{};
    const int ng = (int)T.size();
    c.n_grids = ng;
    bool col = true;   // column mode for every grid
    for (int g = 0; g < ng; ++g) {
        const NsTable& N = T[g];
        CgGrid& C = c.g[g];
        for (int e = 0; e < 3; ++e) C.shape[e] = N.shape[e];
        C.col0 = (int32_t)N.col0;
        C.node0 = N.node0;
        if (!N.on) continue;
        const std::vector<std::array<int, 3>>& offs = N.offs;
        if ((int)offs.size() > CG_MAX_OFF) { why = "normal stencil wider than CG_MAX_OFF"; return false; }
        int h[3] = {0, 0, 0};
        for (const auto& o : offs)
            for (int e = 0; e < 3; ++e) h[e] = std::max(h[e], std::abs(o[e]));
        const int S2 = N.shape[2];
        if (S2 > 4 * CG_MAXI) { why = "more than 64 nodes along the last grid dimension"; return false; }
        C.hy = h[0];
        C.hx = h[1];
        C.ht = h[2];
        C.tpad = (S2 & 1) ? S2 : S2 + 1;
        C.wx = CG_TX + 2 * C.hx;
        C.front = C.ht;
        C.noff = (int)offs.size();
        for (int o = 0; o < C.noff; ++o) {
            C.loff[o] = (offs[o][0] * C.wx + offs[o][1]) * C.tpad + offs[o][2];
            for (int e = 0; e < 3; ++e) C.ooff[o][e] = (int8_t)offs[o][e];
        }
        for (int e = 0; e < 3; ++e) {
            C.K[e] = N.K[e];
            C.ncls[e] = N.ncls[e];
        }
        // column mode: dim 2 ≤ CG_MAXT, |dt| ≤ 2, ≤ CG_MAX_GRP (dy, dx) groups
        std::vector<std::array<int, 2>> grp;
        for (const auto& o : offs)
            if (std::find(grp.begin(), grp.end(), std::array<int, 2>{o[0], o[1]}) == grp.end()) grp.push_back({o[0], o[1]});
        col = col && S2 <= CG_MAXT && C.ht <= 2 && (int)grp.size() <= CG_MAX_GRP;
    }
    // geometry: column mode — strips of ty rows streamed 4·rpw rows per step through a ring of
    // 4·rpw + 2·hy rows (rpw = 4 for 2-D grids); tile mode — tiles of as many rows as
    // 4·CG_MAXI (row, dim-2) items allow
    for (int g = 0; g < ng && col; ++g)
        if (T[g].on) col = c.g[g].wx * c.g[g].tpad <= (c.g[g].shape[2] == 1 ? 2 : CG_NCW) * 64;
    int max3 = 0;   // column mode: the register column length of the grids with dim 2 > 1 (12 or 16)
    for (int g = 0; g < ng; ++g)
        if (T[g].on && c.g[g].shape[2] > 1) max3 = std::max(max3, c.g[g].shape[2] <= 12 ? 12 : CG_MAXT);
    if (!max3) max3 = 12;
    c.maxt3 = max3;
    // strip length: the shortest (multiple of 4, 4..32 rows) whose strips fit one round of two
    // workgroups per CU (the ring's LDS allows two): long strips amortise the 2·hy halo rows, but
    // a second, mostly empty round of strips costs a whole strip time (multigrid level 1 at C4:
    // 8-row strips = 585 workgroups, two rounds; 12-row strips = 387, one).  Grids too large for
    // one round take 32.  LSQ_CG_YS overrides (development).
    int64_t s0max = 1, ntxmax = 1;   // rows / strip columns of the largest grid
    for (int g = 0; g < ng; ++g)
        if (T[g].on && (int64_t)c.g[g].shape[0] * ((c.g[g].shape[1] + CG_TX - 1) / CG_TX) > s0max * ntxmax) {
            s0max = c.g[g].shape[0];
            ntxmax = (c.g[g].shape[1] + CG_TX - 1) / CG_TX;
        }
    int ys3 = 32;
    for (int ys = 4; ys <= 32; ys += 4)
        if ((s0max + ys - 1) / ys * ntxmax <= 2 * (int64_t)std::max(cus, 1)) {
            ys3 = ys;
            break;
        }
    const char* ys_env = getenv("LSQ_CG_YS");
    if (ys_env) ys3 = std::max(4, atoi(ys_env) / 4 * 4);
    int tiles = 0, ldsmax = 0;
    for (int g = 0; g < ng; ++g) {
        CgGrid& C = c.g[g];
        C.tile0 = col ? 0 : tiles;
        if (!T[g].on) continue;
        const int S2 = C.shape[2];
        int back = C.ht;
        C.tc = S2;
        C.nch = 1;
        C.th = 0;
        if (col) {
            C.maxt = S2 == 1 ? 1 : max3;   // register column length: 1, or one length for every 3-D grid
            C.rpw = S2 == 1 ? 4 : 1;
            C.ty = ys3;
            // back pad: column mode reads MAXT + 2·DT values from every column start (zeros past the ring)
            back = std::max(C.ht, C.maxt + 2 - C.tpad);
            C.lds = C.front + (4 * C.rpw + 2 * C.hy) * C.wx * C.tpad + back;
        } else {
            C.ty = std::max(1, std::min(C.shape[0], std::min(48 / S2, 4 * CG_MAXI / S2)));
            C.lds = C.front + (C.ty + 2 * C.hy) * C.wx * C.tpad + back;
            if (chunks && (size_t)C.lds * sizeof(double) > 64 * 1024 && cg_chunk_geometry(C)) c.chunk = 1;
        }
        C.tq = C.tpad;
        if ((size_t)C.lds * sizeof(double) > 64 * 1024) { why = "normal-stencil tile exceeds 64 KB of LDS"; return false; }
        C.nty = (C.shape[0] + C.ty - 1) / C.ty;
        C.ntx = (C.shape[1] + CG_TX - 1) / CG_TX;
        // column mode: strip b of every grid; chunk mode: a workgroup per (tile, chunk)
        tiles = col ? std::max(tiles, C.nty * C.ntx) : tiles + C.nty * C.ntx * C.nch;
        for (int k = 0; k < 2; ++k) {
            C.fd_c[k] = make_fastdiv((uint32_t)std::max(C.tc - k, 1));
            C.fd_ic[k] = make_fastdiv((uint32_t)(CG_TX * std::max(C.tc - k, 1)));
        }
        ldsmax = std::max(ldsmax, C.lds);
        C.fd_pad = make_fastdiv((uint32_t)C.tpad);
        C.fd_row = make_fastdiv((uint32_t)(C.wx * C.tpad));
        C.fd_s2 = make_fastdiv((uint32_t)S2);
        C.fd_int = make_fastdiv((uint32_t)(CG_TX * S2));
    }
    c.ntiles = tiles;
    c.lds_max = ldsmax;
    // 8-wave workgroups for the CG iteration's operator when the strips do not fill the CUs
    // (one box, 4 → 8 waves: C1 67 → 59 µs per iteration; C3, C4 and a rank's window at N = 8
    // within ±1 %, so the 4-wave kernel stays there).  LSQ_CG_W8 = 0 / 1 forces it.
    static const int w8_env = getenv("LSQ_CG_W8") ? atoi(getenv("LSQ_CG_W8")) : -1;
    c.w8 = col && max3 == 12 && (w8_env == 1 || (w8_env < 0 && tiles <= cus));
    c.rw_kt = -1;
    // bits 1.. of colmode: development phase switches (LSQ_CG_DBG: 1 skip the stencil compute,
    // 2 skip the data term, 4 skip the staging loads; results are wrong when set) and 8 (A/B,
    // LSQ_CG_RW_ALT=0): every wave strip walks its rows upwards
    const char* dbg_env = getenv("LSQ_CG_DBG");
    static const int alt_env = getenv("LSQ_CG_RW_ALT") ? atoi(getenv("LSQ_CG_RW_ALT")) : 1;
    c.colmode = col ? 1 | (((dbg_env ? atoi(dbg_env) & 7 : 0) | (alt_env ? 0 : 8)) << 1) : 0;
    coef.clear();
    coefc.clear();
    // the wave-strip operator (lsqr_cg_rw.inc): column mode, 3-D grids of ≤ 12 nodes along dim 2,
    // every (dy, dx) group inside the 5×5 box.  LSQ_CG_RW = 0 keeps the ring kernel (A/B); 2
    // forces the wave-strip kernel on short strips too (tests).
    static const int rw_env = getenv("LSQ_CG_RW") ? atoi(getenv("LSQ_CG_RW")) : 1;
    bool rw_ok = col && rw_env != 0 && max3 == 12;
    int rw_t2 = 1;   // the 3-D grids' common dim-2 length (1: 2-D grids only)
    for (int g = 0; g < ng && rw_ok; ++g) {
        if (!T[g].on) continue;
        // buffer-resource ranges and row offsets are 32-bit: every grid (2-D too) under 2^31 bytes
        if ((int64_t)T[g].shape[0] * T[g].shape[1] * std::max(T[g].shape[2], 1) * 8 >= ((int64_t)1 << 31))
            rw_ok = false;
        if (T[g].shape[2] > 1) {
            if (rw_t2 > 1 && T[g].shape[2] != rw_t2) rw_ok = false;
            rw_t2 = T[g].shape[2];
        }
    }
    if (rw_t2 < 4) rw_ok = rw_ok && rw_t2 == 1;   // instantiated: 2-D only, or 4 … 12 nodes along dim 2
    for (int g = 0; g < ng; ++g) {
        const NsTable& N = T[g];
        CgGrid& C = c.g[g];
        if (!N.on) continue;
        const std::vector<std::array<int, 3>>& offs = N.offs;
        // column-mode groups, ordered by dt half-width
        std::vector<std::array<int, 2>> grp;
        std::vector<int> gdt;
        for (int w = 0; w <= 2; ++w) {
            C.ngrp[w] = 0;
            for (const auto& o : offs) {
                const std::array<int, 2> gg = {o[0], o[1]};
                if (std::find(grp.begin(), grp.end(), gg) != grp.end()) continue;
                int dtw = 0;
                for (const auto& o2 : offs)
                    if (o2[0] == o[0] && o2[1] == o[1]) dtw = std::max(dtw, std::abs(o2[2]));
                if (dtw != w) continue;
                grp.push_back(gg);
                gdt.push_back(w);
                ++C.ngrp[w];
            }
        }
        const int MT = C.maxt > 0 ? C.maxt : 1;
        C.rowlen = 0;
        if (col) {
            for (size_t k = 0; k < grp.size(); ++k) {
                C.gdy[k] = grp[k][0];
                C.gl[k] = grp[k][1] * C.tpad;
                C.gdx[k] = grp[k][1];
                C.gc[k] = C.rowlen;
                C.rowlen += MT * (2 * gdt[k] + 1);
            }
        }
        for (const auto& o : offs)   // the wave-strip path's slots: 3-D grids the diamond, ±1 dt (centre
                                     // ±2); 2-D grids the 5×5 box
            if (N.shape[2] > 1 ? std::abs(o[0]) + std::abs(o[1]) > 2 ||
                                     std::abs(o[2]) > rw_dt(rw_slot_of(o[0], std::max(-2, std::min(2, o[1]))))
                               : std::abs(o[0]) > 2 || std::abs(o[1]) > 2)
                rw_ok = false;
        C.coef0 = (int)coef.size();
        coef.insert(coef.end(), N.coef.begin(), N.coef.end());
        C.coefc0 = (int)coefc.size();
        if (!col) continue;
        coefc.resize(coefc.size() + (size_t)C.ncls[0] * C.ncls[1] * C.rowlen, 0.0);
        const int S2 = C.shape[2];
        for (int cy = 0; cy < C.ncls[0]; ++cy)
            for (int cx = 0; cx < C.ncls[1]; ++cx) {
                double* crow = coefc.data() + C.coefc0 + (size_t)(cy * C.ncls[1] + cx) * C.rowlen;
                for (int tt = 0; tt < S2; ++tt) {
                    const double* row = N.row(cy, cx, cls_of(tt, S2, N.K[2], N.ncls[2]));
                    for (int o = 0; o < C.noff; ++o) {
                        if (row[o] == 0.0) continue;
                        const int k = (int)(std::find(grp.begin(), grp.end(), std::array<int, 2>{offs[o][0], offs[o][1]}) -
                                            grp.begin());
                        crow[C.gc[k] + tt * (2 * gdt[k] + 1) + offs[o][2] + gdt[k]] = row[o];
                    }
                }
            }
    }
    c.rw = 0;
    c.rw_nwg = 0;
    if (rw_ok) {
        // wave strips: 64 − 2·hx outputs per wave across dim 1.  Every strip must be resident in one
        // round (two 4-wave workgroups per CU: a second round adds a whole strip time — C4 with
        // 568 workgroups for 512 slots ran 150 µs instead of ~95): the 2-D grids (blocks of
        // RW_RB rows, a few µs each) take an eighth of the slots when 3-D grids are present, the
        // 3-D grids the rest in proportion to their nodes, rows split to fit.
        const int64_t B = 8 * (int64_t)std::max(cus, 1);
        int64_t work3 = 0, waves2 = 0;
        for (int g = 0; g < ng; ++g)
            if (T[g].on && c.g[g].shape[2] > 1) work3 += (int64_t)c.g[g].shape[0] * c.g[g].shape[1] * c.g[g].shape[2];
        int64_t n2 = 0;
        for (int g = 0; g < ng; ++g)
            if (T[g].on && c.g[g].shape[2] == 1) ++n2;
        for (int pass = 0; pass < 2; ++pass)   // 2-D grids first (their waves come off the 3-D budget)
            for (int g = 0; g < ng; ++g) {
                CgGrid& C = c.g[g];
                if (!T[g].on || (pass == 0) != (C.shape[2] == 1)) continue;
                if (C.hy > 2 || C.hx > 2) rw_ok = false;
                const int S0 = C.shape[0], S1 = C.shape[1];
                C.rw_nsx = (S1 + (64 - 2 * C.hx) - 1) / (64 - 2 * C.hx);
                C.rw_sx = (S1 + C.rw_nsx - 1) / C.rw_nsx;
                if (C.shape[2] == 1) {
                    const int64_t target = std::max<int64_t>(1, (work3 ? B / 8 : B - 8 * n2) / n2);
                    const int64_t nb = (int64_t)C.rw_nsx * ((S0 + RW_RB - 1) / RW_RB);
                    C.rw_ry = RW_RB * (int)std::max<int64_t>(1, (nb + target - 1) / target);
                } else {
                    const int64_t B3 = std::max<int64_t>(B - waves2 - 8 * ng, C.rw_nsx);
                    const int64_t waves = std::max<int64_t>(C.rw_nsx, B3 * ((int64_t)S0 * S1 * C.shape[2]) / std::max<int64_t>(work3, 1));
                    const int64_t nry = std::max<int64_t>(1, waves / C.rw_nsx);
                    // at least RYMIN rows (round 5: 3; 4 before the strips walked alternate
                    // directions, when each strip's four halo rows came from HBM; one rank's window
                    // at N = 8: 3 rows 39 µs vs 4 rows 44 µs, gpurun_out/r5t)
                    static const int rymin = getenv("LSQ_CG_RW_RYMIN") ? atoi(getenv("LSQ_CG_RW_RYMIN")) : 3;   // A/B
                    C.rw_ry = std::max<int>(rymin, (int)((S0 + nry - 1) / nry));
                }
                static const int ry_env = getenv("LSQ_CG_RW_RY") ? atoi(getenv("LSQ_CG_RW_RY")) : 0;   // development
                if (ry_env > 0 && C.shape[2] > 1) C.rw_ry = ry_env;
                // strips shorter than 8 rows load more halo rows (4 per strip) than they compute; with
                // the class-compressed table they still win while the strips fill a quarter of the
                // slots (one box, minimum heights 4 vs 8: C3 51.9 vs 53 µs, one rank's window at
                // N = 4 / 8 6.6 k vs 6.25 k / 9.56 k vs 8.78 k CGNR it/s, C4's multigrid level 1), and
                // lose on grids that leave the machine idle (C1, 96 strips: 35 vs 23 µs)
                static const int minry = getenv("LSQ_CG_RW_MINRY") ? atoi(getenv("LSQ_CG_RW_MINRY")) : 8;   // development
                const int64_t strips = (int64_t)C.rw_nsx * ((S0 + C.rw_ry - 1) / C.rw_ry);
                if (C.shape[2] > 1 && C.rw_ry < minry && strips < B / 4 && rw_env != 2) rw_ok = false;
                C.rw_nry = (S0 + C.rw_ry - 1) / C.rw_ry;
                C.rw_chunk = (int)(((int64_t)C.rw_nsx * C.rw_nry + 7) / 8);
                if (C.shape[2] == 1) waves2 += 8 * (int64_t)C.rw_chunk;
            }
        int64_t per_xcd = 0;
        for (int g = 0; g < ng; ++g)
            if (T[g].on) per_xcd += c.g[g].rw_chunk;
        if (rw_ok) {
            c.rw = rw_t2;
            c.rw_nwg = (int)(8 * ((per_xcd + RW_NW - 1) / RW_NW));
            // one class row per dim-2 boundary class where the 3-D grids share a 5-class layout
            // (K[2] = 2: the smooth_fit dz grid's second time derivative); instantiated for 12 epochs
            static const int kt_env = getenv("LSQ_CG_RW_KT") ? atoi(getenv("LSQ_CG_RW_KT")) : 1;   // A/B
            c.rw_kt = kt_env != 0 && rw_t2 == 12 ? 2 : -1;
            for (int g = 0; g < ng; ++g)
                if (T[g].on && c.g[g].shape[2] > 1 && !(T[g].K[2] == 2 && T[g].ncls[2] == 5)) c.rw_kt = -1;
            // the kernel's class table: per dim-0 class of the interior dim-1 class, every slot's
            // taps for every t (3-D: rw_off layout; 2-D: one value per slot)
            for (int g = 0; g < ng; ++g) {
                const NsTable& N = T[g];
                CgGrid& C = c.g[g];
                if (!N.on) continue;
                const int S2 = C.shape[2], NC = S2 > 1 ? rw_nc(S2, c.rw_kt) : 1, len = rw_rowlen(NC);
                C.rwc0 = (int)coefc.size();
                // 3-D grids: ncls[0] more rows after these, the same classes mirrored in dim 0 (slot
                // (dy, dx) holds the taps of (−dy, dx)) for the strips that walk their rows downwards
                coefc.resize(coefc.size() + (size_t)C.ncls[0] * len * (S2 > 1 ? 2 : 1), 0.0);
                for (int cy = 0; cy < C.ncls[0]; ++cy) {
                    double* r = coefc.data() + C.rwc0 + (size_t)cy * len;
                    for (int tt = 0; tt < S2; ++tt) {
                        const double* row = N.row(cy, C.K[1], cls_of(tt, S2, N.K[2], N.ncls[2]));
                        const int tc = S2 > 1 ? rw_tc(tt, S2, c.rw_kt) : 0;   // rows shared by a class coincide
                        for (int o = 0; o < C.noff; ++o) {
                            const int dy = offs_of(N, o, 0), dx = offs_of(N, o, 1), dt = offs_of(N, o, 2);
                            if (S2 > 1) {
                                const int sl = rw_slot_of(dy, dx), sm = rw_slot_of(-dy, dx);
                                r[rw_off(sl, NC) + tc * (2 * rw_dt(sl) + 1) + dt + rw_dt(sl)] = row[o];
                                r[(size_t)C.ncls[0] * len + rw_off(sm, NC) + tc * (2 * rw_dt(sm) + 1) + dt + rw_dt(sm)] =
                                    row[o];
                            } else {
                                r[(dy + 2) * 5 + dx + 2] = row[o];
                            }
                        }
                    }
                }
            }
        }
    }
    if (col) {   // k_cg_xedge items: rows × dim-1 edge positions × dim 2, all grids
        int64_t items = 0;
        for (int g = 0; g < ng; ++g) {
            const CgGrid& C = c.g[g];
            if (!T[g].on) continue;
            const int ne = C.ncls[1] == C.shape[1] ? C.shape[1] : 2 * C.K[1];
            items += (int64_t)C.shape[0] * ne * C.shape[2];
        }
        c.pad[0] = (int)std::max<int64_t>(1, (items * 8 + BLOCK - 1) / BLOCK);   // k_cg_xedge<8> (multigrid)
        // the CG iteration runs the pass beside the data rows with 8 lanes per item (short gather
        // chains; measured on one box, 1 → 8 lanes: C4 495 → 477 µs per iteration, C3 185 → 177,
        // C1 71 → 67, one rank's window at N = 8 158 → 137); LSQ_CG_XE=1: one lane per item
        static const int xe = getenv("LSQ_CG_XE") ? atoi(getenv("LSQ_CG_XE")) : 8;
        c.pad[1] = xe == 1 ? 1 : 8;
        c.nedge = c.pad[1] == 8 ? c.pad[0] : (int)std::max<int64_t>(1, (items + BLOCK - 1) / BLOCK);
    }
    return true;
}

// Build S.cgh, the coefficient tables and the host tables S.cg_ns for the current part row
// scales.  False (+ reason) when the structured normal operator does not apply (then method 1
// falls back to LSQR).
bool cg_describe(System& S, std::string& why) {
    if (!S.mf) { why = "not a structured stencil system"; return false; }
    const MfDesc& d = S.mfh;
    std::vector<NsTable> T(d.n_grids);
    for (int g = 0; g < d.n_grids; ++g)
        if (!ns_from_parts(d, g, T[g], why, S.cg_scaled)) return false;
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, S.device);
    CgDesc c{};
    std::vector<double> coef, coefc;
    if (!cg_layout(T, cus, c, coef, coefc, why, S.cg_chunks && !S.dist)) return false;
    // field-valued parts: 2-D grids, |offsets| ≤ 2, one row scale
    std::vector<CgVar> var;
    int nvb = 0;
    for (int p = 0; p < d.n_parts; ++p) {
        const MfPart& P = d.p[p];
        if (!P.var) continue;
        const MfGrid& G = d.g[P.grid];
        if (G.shape[2] != 1) { why = "field-valued stencil parts on 3-D grids"; return false; }
        CgVar V{};
        V.S0 = G.shape[0];
        V.S1 = G.shape[1];
        V.col0 = G.col0;
        V.ntpl = P.ntpl;
        V.lo0 = P.lo[0];
        V.hi0 = P.hi[0];
        V.lo1 = P.lo[1];
        V.hi1 = P.hi[1];
        V.nfield = P.nfield;
        V.n_eq = P.n_eq;
        V.F = P.F;
        V.w = P.w;
        V.R = 0;
        for (int t = 0; t < P.ntpl; ++t) {
            V.oy[t] = P.off[t][0];
            V.ox[t] = P.off[t][1];
            V.fsel[t] = P.fsel[t];
            V.val[t] = P.val[t];
            V.R = std::max({V.R, std::abs(V.oy[t]), std::abs(V.ox[t])});
        }
        if (V.R > 2) { why = "field-valued stencil part wider than ±2"; return false; }
        V.R = std::max(V.R, 1);
        V.nty = (V.S0 + CGV_TY - 1) / CGV_TY;
        V.ntx = (V.S1 + CGV_TX - 1) / CGV_TX;
        V.blk0 = nvb;
        nvb += V.nty * V.ntx;
        var.push_back(V);
    }
    // parts with a row scale per (y, x) node (lsq_set_cg_scaled; ns_from_parts left them out of the tables)
    std::vector<CgSc> scg;
    std::vector<CgScPart> scp;
    std::vector<int> scid;
    int64_t wn = 0;
    S.cg_sc.clear();
    S.cg_sc_id.clear();
    for (int g = 0; g < d.n_grids && S.cg_scaled; ++g) {
        const MfGrid& G = d.g[g];
        CgSc C{};
        C.part0 = (int)scp.size();
        for (int qq = 0; qq < G.nparts; ++qq) {
            const int pi = G.part[qq];
            const MfPart& P = d.p[pi];
            if (P.wconst || P.var) continue;
            const std::string who = "stencil part " + std::to_string(pi) + " (grid " + std::to_string(g) + ", rows " +
                                    std::to_string(P.row0) + " to " + std::to_string(P.row0 + P.n_eq - 1) + ")";
            if (S.dist || S.virt || S.comm || S.nranks > 1) {
                why = who + " has per-row scales: lsq_set_cg_scaled is single-GPU, a rank of a distributed, virtual or "
                            "device group keeps LSQR";
                return false;
            }
            if (!c.colmode) {
                why = who + " has per-row scales: lsq_set_cg_scaled runs in column mode only, not in tile or chunk mode "
                            "(16 epochs and more)";
                return false;
            }
            CgScPart Q{};
            Q.ntpl = P.ntpl;
            for (int e = 0; e < 3; ++e) {
                Q.lo[e] = P.lo[e];
                Q.hi[e] = P.hi[e];
            }
            for (int t = 0; t < P.ntpl; ++t) {
                Q.oy[t] = P.off[t][0];
                Q.ox[t] = P.off[t][1];
                Q.ot[t] = P.off[t][2];
                Q.val[t] = P.val[t];
                C.R = std::max({C.R, std::abs(Q.oy[t]), std::abs(Q.ox[t])});
                for (int e = 0; e < 3; ++e)   // k_cg_scaled reads p at every entry of an existing row unchecked
                    if (P.lo[e] + P.off[t][e] < 0 || P.hi[e] - 1 + P.off[t][e] >= G.shape[e]) {
                        why = who + " has per-row scales and rows that reach outside the grid";
                        return false;
                    }
            }
            if (C.R > 2) { why = who + " has per-row scales and reaches beyond ±2 in y or x"; return false; }
            Q.w2 = wn;
            wn += (int64_t)(P.hi[0] - P.lo[0]) * (P.hi[1] - P.lo[1]);
            scp.push_back(Q);
            scid.push_back(pi);
        }
        C.np = (int)scp.size() - C.part0;
        if (!C.np) continue;
        C.S0 = G.shape[0];
        C.S1 = G.shape[1];
        C.S2 = G.shape[2];
        C.col0 = G.col0;
        C.fd_s2 = make_fastdiv((uint32_t)C.S2);
        C.sp = C.S2 | 1;
        for (C.ty = 8; C.ty > 1; C.ty /= 2)   // the largest tile whose image fits 64 KB beside the partials' words
            if (cg_sc_lds(C) + 64 <= 64 * 1024 && C.ty * CGS_TX * C.S2 <= CGS_ITEMS * BLOCK) break;
        if (cg_sc_lds(C) + 64 > 64 * 1024 || C.ty * CGS_TX * C.S2 > CGS_ITEMS * BLOCK) {
            why = "per-row scales: a grid's dim-2 column is too long for k_cg_scaled's tile";
            return false;
        }
        C.nty = (C.S0 + C.ty - 1) / C.ty;
        C.ntx = (C.S1 + CGS_TX - 1) / CGS_TX;
        C.blk0 = nvb;
        nvb += C.nty * C.ntx;
        scg.push_back(C);
    }
    if (!scp.empty()) {   // the fields, and the check that a part's scale does not vary along dim 2
        if (S.cg_scw.n != wn) S.cg_scw.alloc(wn);
        if (S.cg_scp.n != (int64_t)scp.size()) S.cg_scp.alloc((int64_t)scp.size());
        S.cg_scp.upload(scp.data(), (int64_t)scp.size(), S.stream);
        DBuf<int32_t> bad((int64_t)scp.size());
        bad.zero(S.stream);
        for (size_t k = 0; k < scp.size(); ++k) {
            const MfPart& P = d.p[scid[k]];
            const int n0 = P.hi[0] - P.lo[0], n1 = P.hi[1] - P.lo[1], n2 = P.hi[2] - P.lo[2];
            hipLaunchKernelGGL(k_cg_sc_field, dim3(grid_for((int64_t)n0 * n1)), dim3(BLOCK), 0, S.stream, P.row0, n0, n1,
                               n2, P.bstride[0], P.bstride[1], P.bstride[2], S.rs.p, S.cg_scw.p + scp[k].w2, bad.p + k);
        }
        KERNEL_CHECK();
        std::vector<int32_t> hb(scp.size());
        bad.download(hb.data(), (int64_t)scp.size(), S.stream);
        HIP_CHECK(hipStreamSynchronize(S.stream));
        for (size_t k = 0; k < scp.size(); ++k)
            if (hb[k]) {
                const MfPart& P = d.p[scid[k]];
                why = "stencil part " + std::to_string(scid[k]) + " (grid " + std::to_string(P.grid) + ", rows " +
                      std::to_string(P.row0) + " to " + std::to_string(P.row0 + P.n_eq - 1) +
                      ") has per-row scales that differ along dim 2 at one (y, x) node: lsq_set_cg_scaled needs one "
                      "scale per node";
                return false;
            }
    }
    S.cg_sc = std::move(scg);
    S.cg_sc_id = std::move(scid);
    S.cg_ns = std::move(T);
    S.cg_var = std::move(var);
    S.cg_nvb = nvb;
    S.cgh = c;
    if (!S.cgd.p) S.cgd.alloc(1);
    S.cgd.upload(&S.cgh, 1, S.stream);
    if (S.cg_coef.n != std::max<int64_t>((int64_t)coef.size(), 1)) S.cg_coef.alloc(std::max<int64_t>((int64_t)coef.size(), 1));
    S.cg_coef.upload(coef.data(), (int64_t)coef.size(), S.stream);
    if (S.cg_coefc.n != std::max<int64_t>((int64_t)coefc.size(), 1))
        S.cg_coefc.alloc(std::max<int64_t>((int64_t)coefc.size(), 1));
    S.cg_coefc.upload(coefc.data(), (int64_t)coefc.size(), S.stream);
    // columns the data rows touch (byte model of the gathers)
    DBuf<unsigned long long> cnt(1);
    cnt.zero(S.stream);
    hipLaunchKernelGGL(k_count_nonempty, dim3(grid_for(S.ATd.rows)), dim3(BLOCK), 0, S.stream, S.ATd.rows, S.ATd.rp.p,
                       cnt.p);
    KERNEL_CHECK();
    unsigned long long hc = 0;
    HIP_CHECK(hipMemcpyAsync(&hc, cnt.p, sizeof(hc), hipMemcpyDeviceToHost, S.stream));
    HIP_CHECK(hipStreamSynchronize(S.stream));
    S.cg_data_cols = (int64_t)hc;
    return true;
}

// workgroups of the normal-stencil operator of a layout (= its gam partial slots)
int cg_ns_grid(const CgDesc& c) { return c.rw ? c.rw_nwg : 8 * ((c.ntiles + 7) / 8); }
int cg_grid_normal(const System& S) { return cg_ns_grid(S.cgh); }

// tile / chunk mode: the entries all workgroups of one normal launch stage from inside their grids
// (tiles and chunks with their halos, clipped at the grid's faces) — the three dimensions separate
int64_t cg_chunk_staged(const CgDesc& c) {
    int64_t all = 0;
    for (int g = 0; g < c.n_grids; ++g) {
        const CgGrid& C = c.g[g];
        if (!C.noff) continue;
        int64_t ry = 0, rx = 0, rt = 0;
        for (int i = 0; i < C.nty; ++i)
            ry += std::min(C.shape[0], (i + 1) * C.ty + C.hy) - std::max(0, i * C.ty - C.hy);
        for (int i = 0; i < C.ntx; ++i)
            rx += std::min(C.shape[1], (i + 1) * CG_TX + C.hx) - std::max(0, i * CG_TX - C.hx);
        for (int k = 0; k < C.nch; ++k)
            rt += std::min(C.shape[2], (k + 1) * C.shape[2] / C.nch + C.th) - std::max(0, k * C.shape[2] / C.nch - C.th);
        all += ry * rx * rt;
    }
    return all;
}

// q = N_s p, p = z + β p_old (β from betap, else the CG state's) written to pnew (when non-null),
// gam partials pᵀN_s p to part[0, cg_ns_grid(ch)): the wave-strip kernel where the layout allows,
// else the ring kernel (8-wave workgroups when its strips do not fill the CUs)
void cg_launch_ns(const CgDesc& ch, const CgDesc* cd, const double* coefc, hipStream_t stream, const CgState* st,
                  const double* z, const double* pold, double* pnew, double* q, double* part, const double* betap) {
    const size_t lds = sizeof(double) * ch.lds_max;
    const dim3 grid((unsigned)cg_ns_grid(ch));
    if (ch.rw) {
        switch (ch.rw) {
#define RW_CASE(T2)                                                                                              \
    case T2:                                                                                                     \
        hipLaunchKernelGGL(k_cg_normal_rw<T2>, grid, dim3(BLOCK), 0, stream, st, cd, coefc, z, pold, pnew, q, part, \
                           betap);                                                                               \
        break;
            RW_CASE(4) RW_CASE(5) RW_CASE(6) RW_CASE(7) RW_CASE(8) RW_CASE(9) RW_CASE(10) RW_CASE(11)
#undef RW_CASE
        default:   // 12, or 2-D grids only (1)
            if (ch.rw_kt == 2)
                hipLaunchKernelGGL((k_cg_normal_rw<12, 2>), grid, dim3(BLOCK), 0, stream, st, cd, coefc, z, pold, pnew, q,
                                   part, betap);
            else
                hipLaunchKernelGGL(k_cg_normal_rw<12>, grid, dim3(BLOCK), 0, stream, st, cd, coefc, z, pold, pnew, q,
                                   part, betap);
        }
    } else if (ch.w8)
        hipLaunchKernelGGL(k_cg_normal_col8, grid, dim3(512), lds, stream, st, cd, coefc, z, pold, pnew, q, part, betap);
    else if (ch.maxt3 == 12)
        hipLaunchKernelGGL(k_cg_normal_col<12>, grid, dim3(BLOCK), lds, stream, st, cd, coefc, z, pold, pnew, q, part,
                           betap);
    else
        hipLaunchKernelGGL(k_cg_normal_col<CG_MAXT>, grid, dim3(BLOCK), lds, stream, st, cd, coefc, z, pold, pnew, q,
                           part, betap);
}

struct CgGrids {
    int gD, gN, gB;
};

// multigrid preconditioner (mg.inc, included at the end of this namespace)
void mg_precond(System& S, const CgGrids& g, const CgP& P);
void cg_launch_block(System& S, const CgGrids& g, const CgP& P, double* z, const double* lam);
// the direction buffers of S (phase i in p[i]); a step of phase ph reads p_old = the previous
// phase's buffer and writes p_new = its own
CgP cg_pbufs(const System& S) {
    CgP P;
    for (int i = 0; i < CG_XK; ++i) P.p[i] = S.cg_pb[i].p;
    return P;
}
double* cg_pnew(System& S, int ph) { return S.cg_pb[ph].p; }
const double* cg_pold(const System& S, int ph) { return S.cg_pb[(ph + CG_XK - 1) % CG_XK].p; }
double mg_bytes(const System& S, double op0_bytes);
struct MgDistInfo;
bool mg_build(System& S, std::string& why, const MgDistInfo* di = nullptr);
void mg_setup(System& S);


bool cg_use_dmf(const System& S);
// workgroups of the node-block kernels of a CG step: the update (k_cg_block) and level 0's
// multigrid smoothing share one grid (mg_build checks it).  At most 1 024 (one dispatch round at
// their 4–5 waves per SIMD; 2 048 took 1.6–2): C4, three alternating passes, the multigrid solve
// 0.5–2 % faster in each, CGNR + block-Jacobi equal or faster (profiles/r06_bj_grid_ab.txt).
// LSQ_BJ_WG overrides the cap (A/B)
inline int bj_grid_cap() {
    static const int cap = getenv("LSQ_BJ_WG") ? std::max(8, std::min(NPART, atoi(getenv("LSQ_BJ_WG")))) : 1024;
    return cap;
}
CgGrids cg_grids(const System& S, int precond) {
    CgGrids g;
    // data-row workgroups: 4 SELL slices each (matrix-free rows without a SELL copy: as many as the
    // points would make)
    const int64_t nsl = S.Ad.nslices ? S.Ad.nslices : (cg_use_dmf(S) ? (S.dmf.npts + SELL_C - 1) / SELL_C : 0);
    g.gD = (int)std::min<int64_t>((std::max<int64_t>((nsl + 3) / 4, 1) + 7) / 8 * 8, NPART);   // a multiple of 8 (xcd_block)
    g.gN = cg_grid_normal(S);
    g.gB = precond >= 3 ? grid_for(std::max<int64_t>(S.nblk, 1) * BJ_LANES, BLOCK, bj_grid_cap()) : grid_for(S.n_full, BLOCK * 4, NPART);
    return g;
}

void cg_workspace(System& S) {
    const int64_t nf = std::max<int64_t>(S.n_full, 1);
    if (S.cg_x.n != nf) {
        S.cg_x.alloc(nf);
        S.cg_s.alloc(nf);
        S.cg_z.alloc(nf);
        for (auto& b : S.cg_pb) b.alloc(nf);
        S.cg_q.alloc(nf);
    }
    if (S.cg_t.n != std::max<int64_t>(S.mfh.npts, 1)) S.cg_t.alloc(std::max<int64_t>(S.mfh.npts, 1));
    const int npg = cg_grid_normal(S) + (S.cgh.colmode ? S.cgh.nedge : 0) + S.cg_nvb;
    if (S.cg_part_g.n != npg) S.cg_part_g.alloc(npg);
    if (!S.cg_part_r.p) S.cg_part_r.alloc(NPART);
    // the data rows' partials, then the biases'; then (set: more room) the extra rows'
    if (!S.cg_part_t.p) S.cg_part_t.alloc(NPART + ELIM_NPART);
    if (S.xr.on && S.cg_part_t.n < NPART + ELIM_NPART + XR_NPART) {
        graph_cache_drop(&S);
        S.cg_part_t.alloc(NPART + ELIM_NPART + XR_NPART);
    }
    if (!S.cst.p) S.cst.alloc(1);
    if (!S.side) {
        HIP_CHECK(hipStreamCreateWithFlags(&S.side, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreateWithFlags(&S.ev_fork, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&S.ev_join, hipEventDisableTiming));
    }
}

// (Re)build the normal-stencil description when the part row scales changed.  Returns cg_ok.
bool cg_prepare(System& S, int precond) {
    if (!S.dist) refresh_scaling(S, precond == 4 ? 3 : precond);   // rs, part w / wconst; csf = 1/‖A_j‖ (precond 1); ranks: their group
    if (precond >= 3 && !S.blk_valid) block_factor(S);
    std::vector<double> key;
    for (int p = 0; p < S.mfh.n_parts; ++p) {
        key.push_back(S.mfh.p[p].wconst ? S.mfh.p[p].w : NAN);
    }
    // lsq_set_cg_scaled: a part with per-row scales keeps its description until the row scales are refreshed
    // (its field is then stale); −(1 + refreshes) is no row scale
    if (S.cg_scaled)
        for (double& k : key)
            if (std::isnan(k)) k = -(double)(1 + S.rs_gen);
    if (!S.cg_ok || key != S.cg_wkey || S.cgd.p == nullptr) {
        graph_cache_drop(&S);   // captured launches hold the table / description pointers
        mg_free(S.mg);          // the multigrid levels are Galerkin products of these tables
        S.mg = nullptr;
        S.mg_why.clear();
        S.cg_ok = S.mf && cg_describe(S, S.cg_why);
        S.cg_wkey = key;
        S.cg_ready = false;
    }
    if (S.cg_ok) {
        ensure_workspace(S);   // LSQR buffers reused by the init (u, bw, partials, LsqState)
        cg_workspace(S);
        if (precond == 4 && !S.mg && S.mg_why.empty() && !mg_build(S, S.mg_why) && S.mg_why.empty())
            S.mg_why = "multigrid unavailable";
    }
    return S.cg_ok;
}

// update kernel: x += αp, s −= αq, z = M⁻¹s, Σ sᵀz
// p: this step's direction; pold: the previous one (the owed x step, see CgState::pend)
// block-Jacobi update (k_cg_block): x every CG_XK-th step, s −= αq, z = M⁻¹s (× c₂(λ) when lam: the
// multigrid V-cycle's first smoothing step)
constexpr int64_t CG_RC_MAXBLK = 2 << 20;   // node blocks above which k_cg_block reads row and column apart
void cg_launch_block(System& S, const CgGrids& g, const CgP& P, double* z, const double* lam) {
    const int npks = lf_stride(S.blk_kmax * (S.blk_kmax + 1) / 2);
    const uint8_t* live = S.dist ? S.live.p : nullptr;
    // non-temporal bits (LSQ_CG_NT, A/B): 1 factor loads, 2 x stores, 4 s and z stores.  C4, one
    // box: 0 → 0.229–0.239 ms, 1 → 0.215, 4 → 0.215, 5 → 0.206, 7 → 0.208: the 0.33 GB factor
    // stream and the written vectors no longer displace q and s from the caches
    static const int nt = getenv("LSQ_CG_NT") ? atoi(getenv("LSQ_CG_NT")) & 7 : 5;
    using BlkK = void (*)(const CgState*, int64_t, int, BlkAffine, int, const int64_t*, const int32_t*, const lf_t*,
                          CgP, const double*, double*, double*, double*, double*, const uint8_t*, const double*, int);
    static const int bdbg = getenv("LSQ_CG_BLOCK_DBG") ? atoi(getenv("LSQ_CG_BLOCK_DBG")) : 0;   // development
    static const BlkK k12[8] = {k_cg_block<true, 12, 0>, k_cg_block<true, 12, 1>, k_cg_block<true, 12, 2>,
                                k_cg_block<true, 12, 3>, k_cg_block<true, 12, 4>, k_cg_block<true, 12, 5>,
                                k_cg_block<true, 12, 6>, k_cg_block<true, 12, 7>};
    // the factor's row and column read separately (bit 8 of the kernel's NT): LSQ_CG_BLOCK_RC = 0 /
    // 1 forces either form; by default the separate reads above CG_RC_MAXBLK node blocks (C5), one
    // read per entry below (C4) — DESIGN.md §5, round 6
    static const int rc_env = getenv("LSQ_CG_BLOCK_RC") ? atoi(getenv("LSQ_CG_BLOCK_RC")) : -1;
    const bool two = rc_env == 0 || (rc_env < 0 && S.nblk > CG_RC_MAXBLK);
    if (S.blk_affine && S.blk_kmax <= 12 && two && nt == 5)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cg_block<true, 12, 13>), dim3(g.gB), dim3(BLOCK), 0, S.stream, S.cst.p, S.nblk,
                           npks, S.blk_aff, S.blk_kmax, S.blk_ptr.p, S.blk_full.p, S.blk_Lf.p, P, S.cg_q.p, S.cg_x.p,
                           S.cg_s.p, z, S.cg_part_r.p, live, lam, bdbg);
    else if (S.blk_affine && S.blk_kmax <= 12)
        hipLaunchKernelGGL(k12[nt], dim3(g.gB), dim3(BLOCK), 0, S.stream, S.cst.p, S.nblk, npks, S.blk_aff, S.blk_kmax,
                           S.blk_ptr.p, S.blk_full.p, S.blk_Lf.p, P, S.cg_q.p, S.cg_x.p, S.cg_s.p, z,
                           S.cg_part_r.p, live, lam, bdbg);
    else if (S.blk_affine)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cg_block<true, BJ_LANES>), dim3(g.gB), dim3(BLOCK), 0, S.stream, S.cst.p,
                           S.nblk, npks, S.blk_aff, S.blk_kmax, S.blk_ptr.p, S.blk_full.p, S.blk_Lf.p, P,
                           S.cg_q.p, S.cg_x.p, S.cg_s.p, z, S.cg_part_r.p, live, lam, 0);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cg_block<false, BJ_LANES>), dim3(g.gB), dim3(BLOCK), 0, S.stream, S.cst.p,
                           S.nblk, npks, S.blk_aff, S.blk_kmax, S.blk_ptr.p, S.blk_full.p, S.blk_Lf.p, P,
                           S.cg_q.p, S.cg_x.p, S.cg_s.p, z, S.cg_part_r.p, live, lam, 0);
}

void cg_launch_precond(System& S, const CgGrids& g, int precond) {
    const CgP P = cg_pbufs(S);
    if (precond == 4) {
        mg_precond(S, g, P);
        return;
    }
    if (precond == 3) {
        cg_launch_block(S, g, P, S.cg_z.p, nullptr);
    } else {
        hipLaunchKernelGGL(k_cg_jacobi, dim3(g.gB), dim3(BLOCK), 0, S.stream, S.cst.p, S.n_full, S.csf.p, P, S.cg_q.p,
                           S.cg_x.p, S.cg_s.p, S.cg_z.p, S.cg_part_r.p);
    }
}

// t = Ad·p (+ partials ‖t‖² in column mode): tile mode forms p = z + β p_old on the fly (it runs
// before the normal kernel), column mode reads the p the normal kernel wrote
// (tile and chunk mode under lsq_set_cg_tile_dmf too: cg_tile_dmf)
bool cg_use_dmf(const System& S) { return S.dmf.ok && (S.cgh.colmode || S.cg_tile_dmf); }
// tile or chunk mode on matrix-free data rows: column mode's step order around k_cg_normal<false>
inline bool cg_tile_dmf(const System& S) { return !S.cgh.colmode && cg_use_dmf(S); }
// the step runs NORMAL, AD, …, ATQ (else tile mode's AD, NORMAL)
inline bool cg_col_order(const System& S) { return S.cgh.colmode || cg_use_dmf(S); }

// ---- the plain step's stages, in column mode's launch order (DESIGN.md §CGNR, "The step's stages") --
// q = N p (cg_launch_apply): NORMAL, AD, the elimination's E0 … E3 (elim_nbk), XR_FWD and XR_ATQ
// (xr_active), ATQ; tile mode runs AD, then NORMAL (which adds ATd·t), and nothing else — unless its data
// rows are matrix-free (cg_tile_dmf): then column mode's order, without the extra rows.  Then
// cg_launch_update: ALPHA, PRECOND, BETA.  BEGIN stands before the step's first launch, SCALED0 inside
// NORMAL in front of k_cg_scaled (with it in the mask, NORMAL's time is that kernel's).
enum CgStage {
    CG_BEGIN, CG_SCALED0, CG_NORMAL, CG_AD, CG_E0, CG_E1, CG_E2, CG_E3, CG_XR_FWD, CG_XR_ATQ, CG_ATQ, CG_ALPHA, CG_PRECOND,
    CG_BETA, CG_NSTAGE
};
constexpr unsigned cg_bit(int stage) { return 1u << stage; }

// The profilers' stage marks: an event behind every stage of mask, in launch order (ev holds enough
// for every repetition; stage names the ones recorded so far).  The solver passes no marks.
struct CgMarks {
    unsigned mask = 0;
    bool bias_path = false;   // both eliminations in the step: E0 … E3 stand on the bias / slope path, not on the grids'
    std::vector<hipEvent_t> ev;
    std::vector<int> stage;
};
inline void cg_mark(CgMarks* m, int stage, hipStream_t st) {
    if (!m || !(m->mask & cg_bit(stage))) return;
    HIP_CHECK(hipEventRecord(m->ev[m->stage.size()], st));
    m->stage.push_back(stage);
}

void cg_mark_scaled(CgMarks* m, hipStream_t st) { cg_mark(m, CG_SCALED0, st); }

#include "bias.inc"
#include "sgrid.inc"
#include "xrows.inc"

// the data rows' row scales in the matrix-free point order (per solve)
void cg_dmf_prepare(System& S) {
    if (!cg_use_dmf(S)) return;
    hipLaunchKernelGGL(k_dmf_rs, dim3(grid_for(S.dmf.npts)), dim3(BLOCK), 0, S.stream, S.dmf.npts, S.dmf_perm.p,
                       S.rs.p, reinterpret_cast<double4*>(S.dmf_pt.p));
    KERNEL_CHECK();
    if (bias_active(S)) bias_prepare(S);
    if (sgrid_active(S)) sgrid_prepare(S);
}

// the data rows' partials of pᵀNp: Σt² per workgroup, then (biases set) −Σ_j s_j²/D_j, then (extra
// rows set) their Σt_x² per workgroup
int cg_nt(const System& S, const CgGrids& g) {
    return cg_col_order(S) ? g.gD + elim_nbk(S) + (xr_active(S) ? S.xr.nbk : 0) : 0;
}

// extra rows set: t_x = W_x X p and q += Xᵀ W_x t_x, after q = N_s p (and its x-edge correction) and
// before the node gather whose workgroup 0 sums the partials (xrows.inc)
void cg_launch_xr(System& S, const CgGrids& g, const double* pnew, CgMarks* marks = nullptr) {
    if (!xr_active(S)) return;
    xr_launch_fwd(S, S.cst.p, nullptr, pnew, 1.0, S.cg_part_t.p + g.gD + elim_nbk(S));
    cg_mark(marks, CG_XR_FWD, S.stream);
    xr_launch_atq(S, S.cst.p, S.cg_q.p);
    cg_mark(marks, CG_XR_ATQ, S.stream);
}

// biases or sensor grids set: td ← W(I − Q)W A_d p between Ad·p and q += Adᵀ td (bias.inc, sgrid.inc)
void cg_launch_bias(System& S, const CgGrids& g, CgMarks* marks = nullptr) {
    if (elim_nbk(S)) elim_launch_step(S, S.cst.p, S.cg_t.p, S.cg_part_t.p + g.gD, marks);
}

// t = Ad·p and its elimination (elim_nbk needs the matrix-free data rows)
void cg_launch_data(System& S, const CgGrids& g, const double* pold, const double* pnew, CgMarks* marks = nullptr) {
    if (cg_use_dmf(S))
        hipLaunchKernelGGL(k_cg_dmf_ad, dim3(g.gD), dim3(BLOCK), 0, S.stream, S.cst.p, S.dmf,
                           reinterpret_cast<const double4*>(S.dmf_pt.p), pnew, S.cg_t.p, S.cg_part_t.p);
    else if (S.cgh.colmode)
        hipLaunchKernelGGL(k_cg_data, dim3(g.gD), dim3(BLOCK), 0, S.stream, S.cst.p, S.mfh.npts, S.Ad.nslices,
                           S.Ad.sp.p, S.Ad.ci.p, S.Ad.val.p, pnew, nullptr, S.cg_t.p, S.cg_part_t.p);
    else
        hipLaunchKernelGGL(k_cg_data, dim3(g.gD), dim3(BLOCK), 0, S.stream, S.cst.p, S.mfh.npts, S.Ad.nslices,
                           S.Ad.sp.p, S.Ad.ci.p, S.Ad.val.p, S.cg_z.p, pold, S.cg_t.p, nullptr);
    cg_mark(marks, CG_AD, S.stream);
    cg_launch_bias(S, g, marks);
}

// k_cg_dmf_atq: 4 strips of 64 nodes per workgroup, the grid a multiple of 8 (xcd_block);
// k_cg_dmf_atq_long: 4 (strip, chunk of the column) units per workgroup
dim3 cg_atq_grid(const System& S) {
    const int64_t nch = S.dmf.S2 > CG_MAXT ? (S.dmf.S2 + DMF_TC - 1) / DMF_TC : 1;
    const int64_t strips = (int64_t)S.dmf.S0 * ((S.dmf.S1 + 63) / 64) * nch;
    return dim3((unsigned)(((strips + BLOCK / 64 - 1) / (BLOCK / 64) + 7) / 8 * 8));
}

// q += Adᵀ td by node (matrix-free data rows); ast set: α from the partials in workgroup 0 (the
// production step).  Streaming the cell rows per wave instead measured slower (DESIGN.md §3, multigrid:
// "measured and dropped")
void cg_launch_dmf_atq(const System& S, const CgState* st, const double* td, double* q, CgState* ast = nullptr,
                       const double* apg = nullptr, int ang = 0, const double* apt = nullptr, int ant = 0) {
    const double4* P = reinterpret_cast<const double4*>(S.dmf_pt.p);
    const dim3 grid = cg_atq_grid(S);
    if (S.dmf.S2 <= 12)
        hipLaunchKernelGGL(k_cg_dmf_atq<12>, grid, dim3(BLOCK), 0, S.stream, st, S.dmf, S.dmf_cell.p, P, td, q, ast, apg,
                           ang, apt, ant);
    else if (S.dmf.S2 <= CG_MAXT)
        hipLaunchKernelGGL(k_cg_dmf_atq<CG_MAXT>, grid, dim3(BLOCK), 0, S.stream, st, S.dmf, S.dmf_cell.p, P, td, q,
                           ast, apg, ang, apt, ant);
    else
        hipLaunchKernelGGL(k_cg_dmf_atq_long, grid, dim3(BLOCK), 0, S.stream, st, S.dmf, S.dmf_cell.p, P, td, q, ast,
                           apg, ang, apt, ant);
}

void cg_launch_atdq(System& S) {
    if (cg_use_dmf(S)) {
        cg_launch_dmf_atq(S, S.cst.p, S.cg_t.p, S.cg_q.p);
        return;
    }
    hipLaunchKernelGGL(k_cg_atdq, dim3((unsigned)((S.mfh.nodes + CG_AR * BLOCK - 1) / (CG_AR * BLOCK))), dim3(BLOCK), 0,
                       S.stream, S.cst.p,
                       S.mfd.p, S.ATd.rp.p, S.ATd.ci.p, S.ATd.val.p, S.cg_t.p, S.cg_q.p);
}

void cg_launch_xedge(System& S, const CgGrids& g, const double* pnew, hipStream_t st) {
    if (S.cgh.pad[1] == 8)
        hipLaunchKernelGGL(k_cg_xedge<8>, dim3(S.cgh.nedge), dim3(BLOCK), 0, st, S.cst.p, S.cgd.p, S.cg_coef.p, pnew,
                           S.cg_q.p, S.cg_part_g.p + g.gN);
    else
        hipLaunchKernelGGL(k_cg_xedge<1>, dim3(S.cgh.nedge), dim3(BLOCK), 0, st, S.cst.p, S.cgd.p, S.cg_coef.p, pnew,
                           S.cg_q.p, S.cg_part_g.p + g.gN);
}

// xedge = false: the caller launches k_cg_xedge itself (cg_launch_iteration runs it on S.side)
void cg_launch_normal(System& S, const CgGrids& g, const double* pold, double* pnew, bool xedge = true,
                      CgMarks* marks = nullptr) {
    const size_t lds = sizeof(double) * S.cgh.lds_max;
    if (S.cgh.colmode) {
        cg_launch_ns(S.cgh, S.cgd.p, S.cg_coefc.p, S.stream, S.cst.p, S.cg_z.p, pold, pnew, S.cg_q.p, S.cg_part_g.p,
                     nullptr);
        if (xedge) {
            cg_launch_xedge(S, g, pnew, S.stream);
            cg_launch_var(S, pnew, S.cg_q.p, S.cg_part_g.p + g.gN + S.cgh.nedge, S.stream, S.cst.p, marks);
        }
    } else {   // tile mode, or its tiles cut along dim 2 too (chunk mode): the same arguments, step and partial slots
        const bool atd = !cg_use_dmf(S);   // matrix-free data rows: q = N_s p alone (cg_launch_apply)
        hipLaunchKernelGGL(S.cgh.chunk ? (atd ? k_cg_normal_chunk<true> : k_cg_normal_chunk<false>)
                                       : (atd ? k_cg_normal<true> : k_cg_normal<false>),
                           dim3(g.gN), dim3(BLOCK), lds, S.stream, S.cst.p, S.cgd.p, S.cg_coef.p, S.cg_z.p,
                           pold, pnew, S.cg_q.p, S.ATd.rp.p, S.ATd.ci.p, S.ATd.val.p, S.cg_t.p, S.cg_part_g.p);
        cg_launch_var(S, pnew, S.cg_q.p, S.cg_part_g.p + g.gN, S.stream, S.cst.p);
    }
}

// the normal stencil's partials of pᵀNp (with the x-edge correction's and the field-valued parts')
int cg_ng(const System& S, const CgGrids& g) { return g.gN + (S.cgh.colmode ? S.cgh.nedge : 0) + S.cg_nvb; }

void cg_launch_alpha(System& S, const CgGrids& g) {
    hipLaunchKernelGGL(k_cg_alpha, dim3(1), dim3(BLOCK), 0, S.stream, S.cst.p, S.cg_part_g.p, cg_ng(S, g),
                       S.cg_part_t.p, cg_nt(S, g), S.dist ? S.gsum.p : nullptr);
}

// mode 1: ρ0 of the start; mode 0: the step's β.  A rank of a group reads the all-reduced sᵀz
void cg_launch_beta(System& S, const CgGrids& g, int mode) {
    hipLaunchKernelGGL(k_cg_beta, dim3(1), dim3(BLOCK), 0, S.stream, S.cst.p, S.cg_part_r.p, g.gB, mode,
                       S.dist ? S.gsum.p : nullptr);
}

// everything of q = N p behind the normal stencil: t = Ad·p with its elimination, the extra rows,
// q += Adᵀ t.  Tile mode: t alone, k_cg_normal adds ATd·t
void cg_launch_rows(System& S, const CgGrids& g, const double* pold, const double* pnew, CgMarks* marks = nullptr) {
    cg_launch_data(S, g, pold, pnew, marks);
    if (!cg_col_order(S)) return;
    cg_launch_xr(S, g, pnew, marks);
    cg_launch_atdq(S);
    cg_mark(marks, CG_ATQ, S.stream);
}

// THE plain step, first half: p = z + β p_old and q = N p with every partial of pᵀNp, each stage in
// the order the mode requires.  A term added to the operator is added here (and to the two tuned
// spellings in cg_launch_iteration); the profilers, the test hook and the ranks of a group follow.
void cg_launch_apply(System& S, const CgGrids& g, const double* pold, double* pnew, CgMarks* marks = nullptr) {
    cg_mark(marks, CG_BEGIN, S.stream);
    if (cg_col_order(S)) {   // normal (writes p, q = N_s p) → data (t = Ad p) → q += ATd·t
        cg_launch_normal(S, g, pold, pnew, true, marks);
        cg_mark(marks, CG_NORMAL, S.stream);
        cg_launch_rows(S, g, pold, pnew, marks);
    } else {               // data → normal (adds ATd·t)
        cg_launch_rows(S, g, pold, pnew, marks);
        cg_launch_normal(S, g, pold, pnew);
        cg_mark(marks, CG_NORMAL, S.stream);
    }
}

// the plain step, second half: α, the preconditioned update, β
void cg_launch_update(System& S, const CgGrids& g, int precond, CgMarks* marks = nullptr) {
    cg_launch_alpha(S, g);
    cg_mark(marks, CG_ALPHA, S.stream);
    cg_launch_precond(S, g, precond);
    cg_mark(marks, CG_PRECOND, S.stream);
    cg_launch_beta(S, g, 0);
    cg_mark(marks, CG_BETA, S.stream);
}

// one CG iteration of phase ph (0 … CG_XK − 1): p_old in the previous phase's buffer, p_new to
// phase ph's.  Two tuned, overlapped spellings of the column-mode step, else the plain one.  Single
// systems only: a group's ranks step through group_cg_iteration (lsq_solve and lsq_iterate branch
// on S.dist before they reach cg_solve / cg_iterate).
void cg_launch_iteration(System& S, const CgGrids& g, int ph, int precond) {
    const double* pold = cg_pold(S, ph);
    double* pnew = cg_pnew(S, ph);
    if (S.cgh.colmode && cg_use_dmf(S) && S.cg_var.empty() && S.cg_sc.empty() && S.cgh.pad[1] == 8) {
        // the x-edge correction (q at the dim-1 edge nodes, latency-bound) in the data rows'
        // Ad·p launch (both read p only), then q += Adᵀt with α in the node gather's workgroup 0
        cg_launch_normal(S, g, pold, pnew, false);
        hipLaunchKernelGGL(k_cg_ad_xedge<8>, dim3(g.gD + S.cgh.nedge), dim3(BLOCK), 0, S.stream, S.cst.p, S.dmf,
                           reinterpret_cast<const double4*>(S.dmf_pt.p), pnew, S.cg_t.p, S.cg_part_t.p, g.gD, S.cgd.p,
                           S.cg_coef.p, S.cg_q.p, S.cg_part_g.p + g.gN);
        cg_launch_bias(S, g);
        cg_launch_xr(S, g, pnew);
        cg_launch_dmf_atq(S, S.cst.p, S.cg_t.p, S.cg_q.p, S.cst.p, S.cg_part_g.p, cg_ng(S, g), S.cg_part_t.p,
                          cg_nt(S, g));
        cg_launch_precond(S, g, precond);
        cg_launch_beta(S, g, 0);
        return;
    }
    if (S.cgh.colmode) {
        // the x-edge correction (q at the dim-1 edge nodes, latency-bound) runs beside the data
        // rows' Ad·p, which reads p only; both join before q += Adᵀt
        cg_launch_normal(S, g, pold, pnew, false);
        HIP_CHECK(hipEventRecord(S.ev_fork, S.stream));
        HIP_CHECK(hipStreamWaitEvent(S.side, S.ev_fork, 0));
        cg_launch_xedge(S, g, pnew, S.side);
        cg_launch_var(S, pnew, S.cg_q.p, S.cg_part_g.p + g.gN + S.cgh.nedge, S.side, S.cst.p);
        HIP_CHECK(hipEventRecord(S.ev_join, S.side));
        cg_launch_data(S, g, pold, pnew);
        HIP_CHECK(hipStreamWaitEvent(S.stream, S.ev_join, 0));
        cg_launch_xr(S, g, pnew);   // after the join: the x-edge pass on S.side also updates q
        cg_launch_atdq(S);
    } else {
        cg_launch_apply(S, g, pold, pnew);
    }
    cg_launch_update(S, g, precond);
}

// s0 = Aᵀ(W b − A x0), z0 = M⁻¹ s0, ρ0 (x0 = warm start in compact columns, or null)
// LSQ_SETUP_TRACE=1 (development): the per-solve set-up's phases on stderr, each synchronised
struct SetupTrace {
    bool on = getenv("LSQ_SETUP_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(hipStream_t st, const char* what) {
        if (!on) return;
        HIP_CHECK(hipStreamSynchronize(st));
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "setup %-16s %8.3f ms\n", what, std::chrono::duration<double>(now - t).count() * 1e3);
        t = now;
    }
};

// dbp: b on the device, all m rows in the caller's row order (rows past o.b_rows zero when that is
// set).  setup = false: the multigrid levels were set up by an earlier solve with these row weights
// and mask (lsq_cov_border_solved's later columns); they do not depend on b.
void cg_init_dev(System& S, const double* dbp, const double* h_x0, const lsq_opts& o, int precond, bool no_stop,
                 bool setup, SetupTrace& tr) {
    hipStream_t st = S.stream;
    const Grids lg = grids_for(S);
    const CgGrids g = cg_grids(S, precond);
    const int64_t n = S.G.n;
    S.cg_x.zero(st);
    S.cg_z.zero(st);
    for (auto& b : S.cg_pb) b.zero(st);
    S.cg_q.zero(st);
    S.cg_s.zero(st);
    if (h_x0) {
        DBuf<double> dx0(std::max<int64_t>(n, 1));
        dx0.upload(h_x0, n, st);
        hipLaunchKernelGGL(k_cg_scatter, dim3(grid_for(n)), dim3(BLOCK), 0, st, n, S.keep.p, dx0.p, S.cg_x.p);
        KERNEL_CHECK();
        HIP_CHECK(hipStreamSynchronize(st));
    }
    LsqState ls{};   // the LSQR init kernels only read stop / skip flags in raw mode
    HIP_CHECK(hipMemcpyAsync(S.st.p, &ls, sizeof(ls), hipMemcpyHostToDevice, st));
    CgState h{};
    h.atol = o.atol;
    h.btol = o.btol;
    h.maxit = o.maxit > 0 ? o.maxit : 4 * std::max<int64_t>(n, 1);
    h.no_stop = no_stop ? 1 : 0;
    h.anorm_seed = o.anorm0 > 0.0 ? o.anorm0 : 0.0;
    HIP_CHECK(hipMemcpyAsync(S.cst.p, &h, sizeof(h), hipMemcpyHostToDevice, st));
    tr.mark(st, "upload b");
    cg_dmf_prepare(S);
    static const bool init_dmf = !getenv("LSQ_CG_INIT_DMF") || atoi(getenv("LSQ_CG_INIT_DMF")) != 0;
    if (init_dmf && !h_x0 && cg_use_dmf(S) && o.b_rows > 0 && o.b_rows <= S.mfh.npts && S.dmf.npts == S.mfh.npts) {
        // cold start, b on the data rows only: s0 = A_dᵀ(W_d b_d) by the CG step's node gather
        // instead of two passes over every row of A (≈ 1 ms at C4)
        const int gi = (int)std::min<int64_t>(grid_for(S.dmf.npts), NPART);
        hipLaunchKernelGGL(k_cg_init_dmf, dim3(gi), dim3(BLOCK), 0, st, S.dmf.npts, S.dmf_perm.p,
                           reinterpret_cast<const double4*>(S.dmf_pt.p), dbp, S.cg_t.p, S.part_u.p);
        KERNEL_CHECK();
        // biases set: td ← W(I − Q)W b and ‖r0‖² = bᵀW(I − Q)W b, the reduced problem's
        const int nbk = elim_nbk(S);
        if (nbk) elim_launch_step(S, S.cst.p, S.cg_t.p, S.part_u.p + gi);
        // extra rows: s0 += Xᵀ W_x² b_x, ‖r0‖² = ‖b‖² += ‖W_x b_x‖²
        const int nxk = xr_active(S) ? S.xr.nbk : 0;
        if (nxk) {
            xr_launch_fwd(S, nullptr, dbp, nullptr, -1.0, S.part_u.p + gi + nbk);
            xr_launch_atq(S, nullptr, S.cg_s.p);
        }
        cg_launch_dmf_atq(S, S.cst.p, S.cg_t.p, S.cg_s.p);
        KERNEL_CHECK();
        hipLaunchKernelGGL(k_cg_init, dim3(1), dim3(BLOCK), 0, st, S.cst.p, S.part_u.p, gi + nbk + nxk, S.part_u.p,
                           gi + nbk + nxk, nullptr);
    } else {
        // u = W b − A x0 over all rows (Σu² = ‖r0‖²), then s0 = Aᵀu (raw, full space)
        hipLaunchKernelGGL(k_mf_init_u_for(S), dim3(lg.gD + lg.gS), dim3(BLOCK), 0, st, lg.gD, S.mfh.npts, S.Ad.nslices,
                           S.Ad.sp.p, S.Ad.ci.p, S.Ad.val.p, S.Ad.perm.p, S.mfd.p, h_x0 ? S.cg_x.p : nullptr, S.rs.p,
                           dbp, S.u.p, S.bw.p, S.part_u.p, S.part_b.p);
        KERNEL_CHECK();
        hipLaunchKernelGGL(k_mf_spmtv_for(S), dim3(lg.gM), dim3(BLOCK), 0, st, S.st.p, S.ATd.rp.p, S.ATd.ci.p,
                           S.ATd.val.p, S.mfd.p, S.u.p, S.rs.p, S.csf.p, S.cg_q.p, S.cg_s.p, S.zv.p, S.part_v.p, 1);
        KERNEL_CHECK();
        const int nbk = elim_nbk(S);
        if (nbk) {
            // the reduced problem's u_d = (I − Q) W (b − A_d x0): with e = W²(b − A_d x0) per sorted point
            // and s_j = Σ_{i∈j} e_i, s0 −= A_dᵀ(W² s/D), ‖r0‖² −= Σ s_j²/D_j; the same on W b for ‖b‖
            // (sensor grids: the same with y = M⁻¹ Bᵀ e in place of s / D)
            const int64_t enp = elim_npts(S);
            const double* ew2 = elim_w2(S);
            const int nu = lg.gD + lg.gS, ge = grid_for(enp);
            hipLaunchKernelGGL(k_bias_resid, dim3(ge), dim3(BLOCK), 0, st, enp, S.dmf_perm.p, ew2, dbp, nullptr,
                               S.cg_t.p);
            elim_launch_norm(S, nullptr, S.cg_t.p, S.part_b.p + nu);
            hipLaunchKernelGGL(k_cg_dmf_ad, dim3(g.gD), dim3(BLOCK), 0, st, S.cst.p, S.dmf,
                               reinterpret_cast<const double4*>(S.dmf_pt.p), S.cg_x.p, S.cg_t.p, S.cg_part_t.p);
            hipLaunchKernelGGL(k_bias_resid, dim3(ge), dim3(BLOCK), 0, st, enp, S.dmf_perm.p, ew2, dbp, S.cg_t.p,
                               S.cg_t.p);
            elim_launch_reduce(S, nullptr, S.cg_t.p, S.part_u.p + nu);
            elim_launch_apply(S, nullptr, S.cg_t.p, 1, S.part_u.p + nu);
            cg_launch_dmf_atq(S, S.cst.p, S.cg_t.p, S.cg_s.p);
            KERNEL_CHECK();
        }
        // extra rows: ‖b‖² += ‖W_x b_x‖², u_x = W_x (b_x − X x0), ‖r0‖² += ‖u_x‖², s0 += Xᵀ W_x u_x
        const int nxk = xr_active(S) ? S.xr.nbk : 0;
        if (nxk) {
            const int nu = lg.gD + lg.gS + nbk;
            xr_launch_fwd(S, nullptr, dbp, nullptr, -1.0, S.part_b.p + nu);
            xr_launch_fwd(S, nullptr, dbp, h_x0 ? S.cg_x.p : nullptr, -1.0, S.part_u.p + nu);
            xr_launch_atq(S, nullptr, S.cg_s.p);
            KERNEL_CHECK();
        }
        hipLaunchKernelGGL(k_cg_init, dim3(1), dim3(BLOCK), 0, st, S.cst.p, S.part_u.p, lg.gD + lg.gS + nbk + nxk,
                           S.part_b.p, lg.gD + lg.gS + nbk + nxk, nullptr);
    }
    tr.mark(st, "s0 = A'(Wb-Ax0)");
    if (precond == 4 && setup) {   // multigrid set-up for these row weights (uses q as scratch)
        mg_setup(S);
        S.cg_q.zero(st);
        tr.mark(st, "mg_setup");
    }
    cg_launch_precond(S, g, precond);   // α = 0, p = q = 0, pend = 0: z0 = M⁻¹ s0 and ρ0
    cg_launch_beta(S, g, 1);
    KERNEL_CHECK();
    HIP_CHECK(hipStreamSynchronize(st));
    tr.mark(st, "z0 = M^-1 s0");
    S.cg_parity = 0;
}

void cg_init(System& S, const double* h_b, const double* h_x0, const lsq_opts& o, int precond, bool no_stop) {
    SetupTrace tr;
    const double* dbp = upload_rhs(S, h_b, o, S.stream);
    cg_init_dev(S, dbp, h_x0, o, precond, no_stop, true, tr);
}

// capture + instantiate the graph of `count` (a multiple of CG_XK) iterations from the current
// phase if the cached one does not match (host work: callers run it outside their timed region)
void cg_graph_prepare(System& S, int count, int precond) {
    const CgGrids g = cg_grids(S, precond);
    GraphCache& c = g_cache_cg;
    const int mode = precond * CG_XK + S.cg_parity;
    if (c.exec == nullptr || c.sys != &S || c.key != (const void*)S.cg_x.p || c.batch != count || c.mode != mode) {
        if (c.exec) (void)hipGraphExecDestroy(c.exec);
        c.exec = nullptr;
        hipGraph_t graph;
        HIP_CHECK(hipStreamBeginCapture(S.stream, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < count; ++i) cg_launch_iteration(S, g, (S.cg_parity + i) % CG_XK, precond);
        HIP_CHECK(hipStreamEndCapture(S.stream, &graph));
        HIP_CHECK(hipGraphInstantiate(&c.exec, graph, nullptr, nullptr, 0));
        HIP_CHECK(hipGraphDestroy(graph));
        c.sys = &S;
        c.key = S.cg_x.p;
        c.batch = count;
        c.mode = mode;
    }
}

void cg_run_batch(System& S, int count, bool use_graph, int precond) {
    if (use_graph && count % CG_XK == 0) {   // a whole number of x cycles returns to the phase it started from
        cg_graph_prepare(S, count, precond);
        HIP_CHECK(hipGraphLaunch(g_cache_cg.exec, S.stream));
        return;
    }
    const CgGrids g = cg_grids(S, precond);
    for (int i = 0; i < count; ++i) {
        cg_launch_iteration(S, g, S.cg_parity, precond);
        S.cg_parity = (S.cg_parity + 1) % CG_XK;
    }
    KERNEL_CHECK();
}

// k_cg_scaled's launches: p once, q read and written per column of the grids with scaled parts, and
// every part's field once
double cg_scaled_bytes(const System& S) {
    double b = 8.0 * (double)S.cg_scw.n * (S.cg_sc.empty() ? 0.0 : 1.0);
    for (const CgSc& G : S.cg_sc) b += 24.0 * (double)G.S0 * G.S1 * G.S2;
    return b;
}

// Algorithmic HBM bytes per launch (DESIGN.md §CGNR byte model): out = {data, normal, precond}
void cg_kernel_bytes(const System& S, int precond, double out[3]) {
    const double nf = (double)S.n_full, md = (double)S.mfh.npts, zd = (double)S.GdT.nnz, ne = (double)S.mfh.nodes;
    const double nd = (double)S.cg_data_cols, nk = (double)S.G.n;
    if (cg_use_dmf(S)) {
        // data = Ad·p (point subscripts + scale, p at the data columns, td) + Adᵀ td (cell runs,
        // point subscripts + scale and td again, q RMW at the data columns)
        const double ncell = (double)(S.dmf.S0 - 1) * (double)(S.dmf.S1 - 1);
        out[0] = 40.0 * md + 8.0 * nd + 4.0 * ncell + 40.0 * md + 16.0 * nd;
        if (bias_active(S)) out[0] += bias_step_bytes(S);
        if (sgrid_active(S)) out[0] += sgrid_step_bytes(S);
        out[1] = 32.0 * nf;
        // tile / chunk mode on these rows: chunk mode's staging term, no stored-row terms
        if (S.cgh.chunk) out[1] += 16.0 * ((double)cg_chunk_staged(S.cgh) - nf);
    } else if (S.cgh.colmode) {
        // data = Ad·p (12 B/entry, p gathers, t) + ATd·t (entries, row pointers, t gathers, q RMW)
        out[0] = 12.0 * zd + 8.0 * nd + 8.0 * md + 12.0 * zd + 4.0 * ne + 8.0 * md + 16.0 * nd;
        out[1] = 32.0 * nf;                                       // z, p_old in; p, q out
    } else {
        out[0] = 12.0 * zd + 16.0 * nd + 8.0 * md;
        out[1] = 32.0 * nf + 12.0 * zd + 4.0 * ne + 8.0 * md;
        // chunk mode: z and p_old over every staged image inside its grid (the halos of dim 2 are no
        // longer a tile's own columns), p and q over the owned entries
        if (S.cgh.chunk) out[1] += 16.0 * ((double)cg_chunk_staged(S.cgh) - nf);
    }
    if (xr_active(S)) out[0] += xr_step_bytes(S);
    for (const CgVar& V : S.cg_var)   // field-valued parts: fields + p once, q read and written
        out[1] += (double)V.n_eq * 8.0 * V.nfield + 24.0 * (double)V.S0 * V.S1;
    out[1] += cg_scaled_bytes(S);
    if (precond == 4 && S.mg) {
        out[2] = mg_bytes(S, out[0] + out[1]);
    } else if (precond == 3) {
        const double npks = (double)lf_stride(S.blk_kmax * (S.blk_kmax + 1) / 2);
        // q, s in; s, z out; x every CG_XK-th step (x and four p in, x out: 12 B per step on average;
        // every other step before round 5: x, p_old, p in, x out, 16 B)
        out[2] = 48.0 * nk + (double)sizeof(lf_t) * npks * (double)S.nblk + 8.0 * (double)S.nblk;
    } else {
        out[2] = 56.0 * nf;
    }
}

void cg_fill_stats(const CgState& h, lsq_stats* s) {
    s->iters = h.itn;
    s->istop = h.istop;
    s->method = 1;
    s->r1norm = h.r1norm;
    s->r2norm = h.r1norm;
    s->anorm = h.anorm;
    s->acond = 0.0;   // not estimated by CGNR (istop 3 is never produced)
    s->arnorm = h.arnorm;
    s->xnorm = h.xnorm;
}

#include "mg.inc"

}  // namespace

void bias_values(System& S, const double* dbp);
void sgrid_values(System& S, const double* dbp);

bool cg_available(System& S, int precond) {
    if (precond != 1 && precond != 3 && precond != 4) return false;
    return cg_prepare(S, precond) && (precond != 4 || S.mg);
}

// lsq_set_cg_chunks: the flag cg_describe hands to cg_layout.  A change drops what was built for the
// other layout, as a change of the part row scales does: the description, the captured iterations and
// the multigrid levels; the next cg_prepare lays out afresh.
void cg_set_chunks(System& S, bool on) {
    if (S.cg_chunks == on) return;
    S.cg_chunks = on;
    graph_cache_drop(&S);
    mg_free(S.mg);
    S.mg = nullptr;
    S.mg_why.clear();
    S.cg_ok = false;
    S.cg_why.clear();
    S.cg_ready = false;
}

// lsq_set_cg_scaled: the flag cg_describe hands to ns_from_parts.  A change drops what cg_set_chunks drops.
void cg_set_scaled(System& S, bool on) {
    if (S.cg_scaled == on) return;
    S.cg_scaled = on;
    graph_cache_drop(&S);
    mg_free(S.mg);
    S.mg = nullptr;
    S.mg_why.clear();
    S.cg_ok = false;
    S.cg_why.clear();
    S.cg_ready = false;
    S.cg_sc.clear();
    S.cg_sc_id.clear();
}

// lsq_cg_scaled_info (builds the description if needed): {scaled parts, bytes of their fields, grids with
// scaled parts, workgroups of their launches}; zeros without a CGNR operator or without the key
void cg_scaled_info(System& S, int64_t* out4) {
    std::fill(out4, out4 + 4, (int64_t)0);
    if (!cg_prepare(S, 1)) return;
    out4[0] = (int64_t)S.cg_sc_id.size();
    out4[1] = S.cg_sc.empty() ? 0 : 8 * S.cg_scw.n;
    out4[2] = (int64_t)S.cg_sc.size();
    for (const CgSc& G : S.cg_sc) out4[3] += (int64_t)G.nty * G.ntx;
}

// lsq_set_cg_tile_dmf: read by build_dmf at the formation (the point table of a long column) and by
// cg_use_dmf.  A change drops what cg_set_chunks drops.
void cg_set_tile_dmf(System& S, bool on) {
    if (S.cg_tile_dmf == on) return;
    S.cg_tile_dmf = on;
    graph_cache_drop(&S);
    mg_free(S.mg);
    S.mg = nullptr;
    S.mg_why.clear();
    S.cg_ok = false;
    S.cg_why.clear();
    S.cg_ready = false;
}

// lsq_cg_layout_info: {mode (0 none, 1 column, 2 tile, 3 chunk), ty, tc, chunks of the grid with the
// longest dim 2, its LDS column stride, LDS bytes of the largest tile, workgroups of one normal launch, 0}
void cg_layout_info(System& S, int64_t* out8) {
    std::fill(out8, out8 + 8, (int64_t)0);
    // the geometry does not depend on the row scales: a description that stands is read as it is
    if (!(S.cg_ok && S.cgd.p) && !cg_prepare(S, 1)) return;
    const CgDesc& c = S.cgh;
    const CgGrid* G = nullptr;
    for (int g = 0; g < c.n_grids; ++g)
        if (c.g[g].noff && (!G || c.g[g].shape[2] > G->shape[2])) G = &c.g[g];
    out8[0] = c.colmode ? 1 : c.chunk ? 3 : 2;
    if (G) {
        out8[1] = G->ty;
        out8[2] = G->tc;
        out8[3] = G->nch;
        out8[4] = G->tpad;
    }
    out8[5] = (int64_t)c.lds_max * (int64_t)sizeof(double);
    out8[6] = cg_ns_grid(c);
}

int cg_solve(System& S, const double* h_b, double* h_x, const lsq_opts& o, lsq_stats* stats) {
    const int precond = o.precond;
    const auto t_init = std::chrono::steady_clock::now();
    cg_init(S, h_b, o.use_x0 ? h_x : nullptr, o, precond, false);   // synchronises
    int batch = o.batch > 0 ? o.batch : (precond == 4 ? 4 : 16);   // a multigrid step is ~6 plain ones
    batch = (batch + CG_XK - 1) / CG_XK * CG_XK;   // whole x cycles (graph replay)
    if (o.use_graph) cg_graph_prepare(S, batch, precond);   // instantiation is set-up, not iteration time
    if (getenv("LSQ_SETUP_TRACE"))
        fprintf(stderr, "setup %-16s %8.3f ms (cg_init + graph)\n", "total",
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t_init).count() * 1e3);
    const double init_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_init).count();
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, S.stream));
    CgState h{};
    HIP_CHECK(hipMemcpyAsync(&h, S.cst.p, sizeof(h), hipMemcpyDeviceToHost, S.stream));
    HIP_CHECK(hipStreamSynchronize(S.stream));
    while (!h.stop) {
        cg_run_batch(S, batch, o.use_graph != 0, precond);
        HIP_CHECK(hipMemcpyAsync(&h, S.cst.p, sizeof(h), hipMemcpyDeviceToHost, S.stream));
        HIP_CHECK(hipStreamSynchronize(S.stream));
    }
    hipLaunchKernelGGL(k_cg_xfix, dim3(grid_for(S.n_full)), dim3(BLOCK), 0, S.stream, S.cst.p, S.n_full, cg_pbufs(S),
                       S.cg_x.p);
    HIP_CHECK(hipEventRecord(e1, S.stream));
    const int64_t n = S.G.n;
    DBuf<double> dx(std::max<int64_t>(n, 1));
    hipLaunchKernelGGL(k_cg_gather, dim3(grid_for(n)), dim3(BLOCK), 0, S.stream, n, S.keep.p, S.cg_x.p, dx.p);
    KERNEL_CHECK();
    dx.download(h_x, n, S.stream);
    HIP_CHECK(hipStreamSynchronize(S.stream));
    if (S.bias.nb || S.bias.ng) bias_values(S, S.rhs.p);   // the biases and slopes that belong to this x
    if (S.sgrid.ng) sgrid_values(S, S.rhs.p);              // the sensor grids that belong to this x
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (stats) {
        cg_fill_stats(h, stats);
        stats->time_s = ms * 1e-3;
        stats->setup_s = init_s;
        double b[3];
        cg_kernel_bytes(S, precond, b);
        stats->bytes_per_iter = b[0] + b[1] + b[2];
    }
    S.cg_ready = false;
    return h.istop == 7 ? 1 : 0;
}

int cg_iterate(System& S, const double* h_b, int64_t iters, const lsq_opts& o, lsq_stats* stats) {
    const int precond = o.precond;
    if (!S.cg_ready || S.cg_mode != precond) {
        lsq_opts oo = o;
        oo.maxit = INT64_MAX / 4;
        cg_init(S, h_b, nullptr, oo, precond, true);
        S.cg_ready = true;
        S.cg_mode = precond;
    }
    int batch = o.batch > 0 ? o.batch : 16;
    batch = (batch + CG_XK - 1) / CG_XK * CG_XK;
    if (o.use_graph && iters >= batch) cg_graph_prepare(S, batch, precond);
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, S.stream));
    int64_t left = iters;
    while (left > 0) {
        const int c = (int)std::min<int64_t>(left, batch);
        cg_run_batch(S, c, o.use_graph != 0 && c == batch, precond);
        left -= c;
    }
    HIP_CHECK(hipEventRecord(e1, S.stream));
    if (o.use_graph) cg_graph_prepare(S, batch, precond);   // the next call's batches start from this parity
    CgState h{};
    HIP_CHECK(hipMemcpyAsync(&h, S.cst.p, sizeof(h), hipMemcpyDeviceToHost, S.stream));
    HIP_CHECK(hipStreamSynchronize(S.stream));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (stats) {
        cg_fill_stats(h, stats);
        stats->time_s = ms * 1e-3;
        double b[3];
        cg_kernel_bytes(S, precond, b);
        stats->bytes_per_iter = b[0] + b[1] + b[2];
    }
    return 0;
}

static bool cg_live(const System& S, int precond) { return S.cg_ready && S.cg_mode == precond; }

static void cg_need_live(const System& S, int precond, const char* who) {
    if (!cg_live(S, precond))
        throw std::invalid_argument(std::string(who) + ": needs the live state of lsq_iterate with this precond");
}

// The profilers' core: reps real steps of a live lsq_iterate state (no stop) through the plain step,
// an event behind every stage of mask, so every kernel sees the caches its predecessors leave
// behind.  ms[s] = the mean time from the step's previous mark to the one behind stage s (0 for a
// stage that is not in mask, did not run, or carries the step's first mark).
static void cg_profile_steps(System& S, int reps, int precond, unsigned mask, double ms[CG_NSTAGE],
                             bool bias_path = false) {
    const CgGrids g = cg_grids(S, precond);
    CgMarks m;
    m.mask = mask;
    m.bias_path = bias_path;
    m.ev.resize((size_t)reps * __builtin_popcount(mask));
    for (auto& e : m.ev) HIP_CHECK(hipEventCreate(&e));
    for (int r = 0; r < reps; ++r) {
        cg_launch_apply(S, g, cg_pold(S, S.cg_parity), cg_pnew(S, S.cg_parity), &m);
        cg_launch_update(S, g, precond, &m);
        S.cg_parity = (S.cg_parity + 1) % CG_XK;
    }
    HIP_CHECK(hipStreamSynchronize(S.stream));
    std::fill(ms, ms + CG_NSTAGE, 0.0);
    const size_t per = m.stage.size() / reps;   // every step records the same marks
    for (size_t i = 0; i < m.stage.size(); ++i) {
        if (i % per == 0) continue;
        float a = 0.f;
        HIP_CHECK(hipEventElapsedTime(&a, m.ev[i - 1], m.ev[i]));
        ms[m.stage[i]] += a;
    }
    for (auto& e : m.ev) (void)hipEventDestroy(e);
    for (int s = 0; s < CG_NSTAGE; ++s) ms[s] /= reps;
}

// Per-kernel HIP-event times of one CG iteration's launches and the algorithmic bytes per launch:
// out8 = {ms data, ms normal, ms precond, ms scalars (α + β), bytes data, bytes normal, bytes
// precond, mode bits}.  On a live lsq_iterate state: inside reps real iterations; else reps
// launches of each role on a benign state, which clobbers the iteration state.
void cg_profile(System& S, int reps, int precond, double* out) {
    const CgGrids g = cg_grids(S, precond);
    // bit 0: data rows matrix-free (else stored Ad / ATd); bit 1: wave-strip normal operator; bit 2:
    // column mode (else tile mode); bit 3: chunk mode (tile mode's step on tiles cut along dim 2; bit 2 clear)
    out[7] = (cg_use_dmf(S) ? 1.0 : 0.0) + (S.cgh.rw ? 2.0 : 0.0) + (S.cgh.colmode ? 4.0 : 0.0) +
             (S.cgh.chunk ? 8.0 : 0.0);
    cg_kernel_bytes(S, precond, out + 4);
    if (cg_live(S, precond)) {
        const int rows = cg_col_order(S) ? CG_ATQ : CG_AD;   // the last stage of the data rows' share
        double ms[CG_NSTAGE];
        cg_profile_steps(S, reps, precond,
                         cg_bit(CG_BEGIN) | cg_bit(CG_NORMAL) | cg_bit(rows) | cg_bit(CG_ALPHA) | cg_bit(CG_PRECOND) |
                             cg_bit(CG_BETA),
                         ms);
        out[0] = ms[rows];
        out[1] = ms[CG_NORMAL];
        out[2] = ms[CG_PRECOND];
        out[3] = ms[CG_ALPHA] + ms[CG_BETA];
        return;
    }
    CgState h{};
    h.rho = 1.0; h.beta = 0.5; h.alpha = 1e-3; h.alpha_prev = 1e-3; h.bnorm = 1.0; h.rn2 = 1.0;
    h.maxit = INT64_MAX / 4; h.no_stop = 1; h.atol = h.btol = 1e-12;
    HIP_CHECK(hipMemcpyAsync(S.cst.p, &h, sizeof(h), hipMemcpyHostToDevice, S.stream));
    S.cg_x.zero(S.stream);
    S.cg_z.zero(S.stream);
    for (auto& b : S.cg_pb) b.zero(S.stream);
    S.cg_s.zero(S.stream);
    cg_dmf_prepare(S);
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    for (int k = 0; k < 4; ++k) {
        for (int pass = 0; pass < 2; ++pass) {
            HIP_CHECK(hipEventRecord(e0, S.stream));
            for (int r = 0; r < reps; ++r) {
                if (k == 0)
                    cg_launch_rows(S, g, S.cg_pb[0].p, S.cg_pb[1].p);
                else if (k == 1)
                    cg_launch_normal(S, g, S.cg_pb[0].p, S.cg_pb[1].p);
                else if (k == 2)
                    cg_launch_precond(S, g, precond);
                else {
                    cg_launch_alpha(S, g);
                    cg_launch_beta(S, g, 0);
                }
            }
            HIP_CHECK(hipEventRecord(e1, S.stream));
            HIP_CHECK(hipEventSynchronize(e1));
        }
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        out[k] = ms / reps;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    S.cg_ready = false;
}

// The extra rows' two kernels inside real iterations (cg_profile_steps): out4 = {ms k_xr_fwd, ms
// k_xr_atq (with k_xr_atq_long), ms of the data rows' Ad·p (with its elimination) before them, ms of
// the node gather behind them}, means over reps iterations.
void cg_profile_xr(System& S, int reps, int precond, double* out) {
    cg_need_live(S, precond, "lsq_profile_extra_rows");
    if (!xr_active(S)) throw std::invalid_argument("lsq_profile_extra_rows: no extra rows in the CGNR operator");
    const int data = elim_nbk(S) ? CG_E3 : CG_AD;   // the last stage of t = Ad·p
    double ms[CG_NSTAGE];
    cg_profile_steps(S, reps, precond,
                     cg_bit(CG_NORMAL) | cg_bit(data) | cg_bit(CG_XR_FWD) | cg_bit(CG_XR_ATQ) | cg_bit(CG_ATQ), ms);
    out[0] = ms[CG_XR_FWD];
    out[1] = ms[CG_XR_ATQ];
    out[2] = ms[data];
    out[3] = ms[CG_ATQ];
}

// k_cg_scaled inside real iterations (cg_profile_steps, the mark CG_SCALED0 in front of it): out4 = {ms of
// its launches (one per grid with scaled parts), their algorithmic bytes, ms of the normal kernel, the
// x-edge pass and the field-valued parts in front of them, ms of the whole step}, means over reps iterations.
void cg_profile_scaled(System& S, int reps, int precond, double* out) {
    cg_need_live(S, precond, "lsq_profile_cg_scaled");
    if (S.cg_sc.empty()) throw std::invalid_argument("lsq_profile_cg_scaled: no scaled parts in the CGNR operator");
    double ms[CG_NSTAGE];
    cg_profile_steps(S, reps, precond,
                     cg_bit(CG_BEGIN) | cg_bit(CG_SCALED0) | cg_bit(CG_NORMAL) | cg_bit(CG_BETA), ms);
    out[0] = ms[CG_NORMAL];
    out[1] = cg_scaled_bytes(S);
    out[2] = ms[CG_SCALED0];
    out[3] = ms[CG_SCALED0] + ms[CG_NORMAL] + ms[CG_BETA];
}

// the elimination's four kernels inside real iterations: out4 = ms of the stages E0 … E3
static void cg_profile_elim(System& S, int reps, int precond, double* out, bool bias_path = false) {
    double ms[CG_NSTAGE];
    cg_profile_steps(S, reps, precond,
                     cg_bit(CG_AD) | cg_bit(CG_E0) | cg_bit(CG_E1) | cg_bit(CG_E2) | cg_bit(CG_E3), ms, bias_path);
    std::copy(ms + CG_E0, ms + CG_E3 + 1, out);
}

// The slope elimination's kernels inside real iterations: out8 = {ms chunk pass, ms per-rank sums
// (with the long ranks), ms per-group kernel, ms apply pass, and their algorithmic bytes
// (slope_kernel_bytes)}, means over reps iterations.
void cg_profile_slope(System& S, int reps, int precond, double* out) {
    cg_need_live(S, precond, "lsq_profile_data_slope");
    if (!bias_active(S) || !S.bias.ng) throw std::invalid_argument("lsq_profile_data_slope: no slopes in the CGNR operator");
    cg_profile_elim(S, reps, precond, out, true);   // beside joint sensor grids: the marks on this path (elim_launch_step)
    slope_kernel_bytes(S, out + 4);
}

// The sensor grids' elimination inside real iterations: out8 = {ms of s = Bᵀ td, of z = R⁻ᵀ s, of
// y = R⁻¹ z, of the apply pass, and their algorithmic bytes (sgrid_kernel_bytes)}, means over reps
// iterations.
void cg_profile_sgrid(System& S, int reps, int precond, double* out) {
    cg_need_live(S, precond, "lsq_profile_sensor_grids");
    if (!sgrid_active(S)) throw std::invalid_argument("lsq_profile_sensor_grids: no sensor grids in the CGNR operator");
    cg_profile_elim(S, reps, precond, out);
    sgrid_kernel_bytes(S, out + 4);
}

// The lumping pass of the multigrid set-up in place (lsq_profile_extra_rows_lumping): reps times the
// level-1 blocks of the data rows (k_mg_lump1) and then the extra rows' share (k_mg_lump_xr and its
// long-node kernel), events between them: out2 = {ms of the extra rows' pass, ms of k_mg_lump1}.
// B_1 ends as a set-up leaves it.
void mg_profile_lump_xr(System& S, int reps, double* out2) {
    if (!cg_available(S, 4) || !S.mg || !xr_lumped(S))
        throw std::invalid_argument("lsq_profile_extra_rows_lumping: the multigrid does not carry lumped extra rows");
    cg_workspace(S);
    cg_dmf_prepare(S);
    std::vector<hipEvent_t> ev(3 * reps);
    for (auto& e : ev) HIP_CHECK(hipEventCreate(&e));
    for (int r = 0; r < reps; ++r) {
        HIP_CHECK(hipEventRecord(ev[3 * r], S.stream));
        mg_setup_lump1(S);
        HIP_CHECK(hipEventRecord(ev[3 * r + 1], S.stream));
        mg_setup_lump_xr(S);
        HIP_CHECK(hipEventRecord(ev[3 * r + 2], S.stream));
    }
    HIP_CHECK(hipStreamSynchronize(S.stream));
    double t[2] = {0, 0};
    for (int r = 0; r < reps; ++r) {
        float a = 0.f;
        HIP_CHECK(hipEventElapsedTime(&a, ev[3 * r + 1], ev[3 * r + 2])); t[0] += a;
        HIP_CHECK(hipEventElapsedTime(&a, ev[3 * r], ev[3 * r + 1])); t[1] += a;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    out2[0] = t[0] / reps;
    out2[1] = t[1] / reps;
    S.cg_ready = false;
}

namespace {
__global__ __launch_bounds__(BLOCK) void k_perm_gather(int64_t n, const int32_t* __restrict__ perm,
                                                       const double* __restrict__ src, double* __restrict__ dst) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) dst[i] = src[perm[i]];
}
}  // namespace

// out = G_dataᵀ f over the FULL column space (unweighted data rows, f in data-row order; the
// reference epoch's columns included): the per-node sums of smooth_fit.py:341-347 (count and
// misfit maps), by the matrix-free node gather of k_cg_dmf_atq on the points sorted by cell
void cg_data_colsum(System& S, const double* h_f, double* h_out) {
    if (!S.dmf.ok)
        throw std::invalid_argument("lsq_data_colsum: needs matrix-free data rows (a structured system whose "
                                    "interpolation grids share one (y, x) lattice)");
    const int64_t np = S.dmf.npts, nf = S.n_full;
    DBuf<double> df(std::max<int64_t>(np, 1)), td(std::max<int64_t>(np, 1)), q(std::max<int64_t>(nf, 1));
    DBuf<CgState> st(1);
    st.zero(S.stream);
    df.upload(h_f, np, S.stream);
    hipLaunchKernelGGL(k_perm_gather, dim3(grid_for(np)), dim3(BLOCK), 0, S.stream, np, S.dmf_perm.p, df.p, td.p);
    q.zero(S.stream);
    cg_launch_dmf_atq(S, st.p, td.p, q.p);
    KERNEL_CHECK();
    q.download(h_out, nf, S.stream);
    HIP_CHECK(hipStreamSynchronize(S.stream));
}

// Test hook: q = (AᵀA) p on the structured normal operator (full column space in and out).
void cg_apply_normal(System& S, const double* h_p, double* h_q) {
    const CgGrids g = cg_grids(S, 1);
    const int64_t nf = S.n_full;
    CgState h{};
    h.beta = 0.0;
    HIP_CHECK(hipMemcpyAsync(S.cst.p, &h, sizeof(h), hipMemcpyHostToDevice, S.stream));
    S.cg_z.upload(h_p, nf, S.stream);
    S.cg_pb[0].zero(S.stream);
    cg_dmf_prepare(S);
    cg_launch_apply(S, g, S.cg_pb[0].p, S.cg_pb[1].p);
    KERNEL_CHECK();
    S.cg_q.download(h_q, nf, S.stream);
    HIP_CHECK(hipStreamSynchronize(S.stream));
    S.cg_ready = false;
}

// ---- data biases and slopes (bias.inc, slope.inc): set, clear, read back -------------------------
void bias_clear(System& S) {
    if (!S.bias.on && !S.bias.idx.p) return;
    graph_cache_drop(&S);   // captured iterations hold the step's launches
    S.bias = BiasData{};
    S.cg_ready = false;
}

namespace {
// The layout of the eliminated columns.  h_id: the data rows' bias IDs in the caller's row order
// (null: no biases, the slopes' pseudo-IDs), h_c: 1 / E_bias per ID; h_grp (null: no slopes), h_u,
// h_gc: the rows' slope groups, their coefficients and the groups' c.  Arguments are valid.
// h_sink (null: none): the rows that leave this path for a sensor grid's block (BiasData::sink); they
// form one last ID outside every group with c² = +∞.  Without such a row the layout is the one made
// without h_sink.
void bias_build(System& S, int64_t npts, const int32_t* h_id, int64_t nb, const double* h_c, const int32_t* h_grp,
                const double* h_u, int64_t ng, const double* h_gc, const uint8_t* h_sink = nullptr) {
    std::vector<int32_t> perm(std::max<int64_t>(npts, 1));
    S.dmf_perm.download(perm.data(), npts, S.stream);
    HIP_CHECK(hipStreamSynchronize(S.stream));
    std::vector<int32_t> keep_id, keep_grp;   // the caller's arrays outlive the previous layout
    std::vector<double> keep_c, keep_u, keep_gc;
    std::vector<uint8_t> keep_sink;
    if (h_id) {
        keep_id.assign(h_id, h_id + npts);
        keep_c.assign(h_c, h_c + nb);
    }
    if (h_grp) {
        keep_grp.assign(h_grp, h_grp + npts);
        keep_u.assign(h_u, h_u + 2 * npts);
        keep_gc.assign(h_gc, h_gc + 2 * ng);
    }
    bool has_sink = false;
    for (int64_t i = 0; h_sink && i < npts; ++i) has_sink = has_sink || h_sink[i];
    if (has_sink) keep_sink.assign(h_sink, h_sink + npts);
    bias_clear(S);
    graph_cache_drop(&S);   // captured iterations hold no elimination step yet
    S.cg_ready = false;
    const bool pseudo = !h_id;
    const int64_t ne0 = pseudo ? ng + 1 : nb;   // IDs, or one pseudo-ID per group and one for the rows outside
    const int64_t ne = ne0 + (has_sink ? 1 : 0);   // and the sink
    auto sunk = [&](int64_t i) -> bool { return has_sink && keep_sink[i]; };
    auto eid = [&](int64_t i) -> int32_t {
        if (sunk(i)) return (int32_t)ne0;
        return pseudo ? (h_grp[i] < 0 ? (int32_t)ng : h_grp[i]) : h_id[i];
    };
    // ranks: the IDs that carry points, in ID order; slopes set: by (group, ID), the IDs outside every
    // group last.  The sorted points are indexed stably by rank.
    std::vector<int32_t> cnt(ne + 1, 0), rank_of(ne, -1), rank_id, sgrp(h_grp ? ne : 0, -1);
    for (int64_t i = 0; i < npts; ++i) {
        ++cnt[eid(i)];
        if (h_grp && h_grp[i] >= 0 && !sunk(i)) sgrp[eid(i)] = h_grp[i];
    }
    for (int64_t j = 0; j < ne; ++j)
        if (cnt[j]) rank_id.push_back((int32_t)j);
    int64_t nsr = 0;
    std::vector<int32_t> gseg(ng + 1, 0), rgrp;
    if (h_grp) {
        std::stable_sort(rank_id.begin(), rank_id.end(), [&](int32_t x, int32_t y) {
            return (sgrp[x] < 0 ? ng : sgrp[x]) < (sgrp[y] < 0 ? ng : sgrp[y]);
        });
        for (int32_t j : rank_id)
            if (sgrp[j] >= 0) {
                ++gseg[sgrp[j] + 1];
                rgrp.push_back(sgrp[j]);
                ++nsr;
            }
        for (int64_t g = 0; g < ng; ++g) gseg[g + 1] += gseg[g];
    }
    const int64_t ns = (int64_t)rank_id.size();
    for (int64_t r = 0; r < ns; ++r) rank_of[rank_id[r]] = (int32_t)r;
    std::vector<int32_t> seg(ns + 1, 0), pos(std::max<int64_t>(ns, 1)), idx(std::max<int64_t>(npts, 1)),
        brank(std::max<int64_t>(npts, 1)), rank_pt(std::max<int64_t>(npts, 1));
    std::vector<double> c2(std::max<int64_t>(ns, 1));
    for (int64_t r = 0; r < ns; ++r) {
        seg[r + 1] = seg[r] + cnt[rank_id[r]];
        pos[r] = seg[r];
        if (rank_id[r] == ne0)
            c2[r] = INFINITY;   // the sink: D = +∞
        else
            c2[r] = pseudo ? 0.0 : h_c[rank_id[r]] * h_c[rank_id[r]];
    }
    for (int64_t i = 0; i < npts; ++i) {
        const int32_t r = rank_of[eid(perm[i])];
        rank_pt[i] = r;
        const int32_t k = pos[r]++;
        idx[k] = (int32_t)i;
        brank[k] = r;
    }
    const int64_t nchunk = (npts + BIAS_CHUNK - 1) / BIAS_CHUNK;
    std::vector<int32_t> sbase(std::max<int64_t>(nchunk, 1));
    int64_t nslots = 0, npts3 = 0, nslots3 = 0;
    for (int64_t c = 0; c < nchunk; ++c) {
        const int64_t kb = std::min(npts, (c + 1) * BIAS_CHUNK);
        const int32_t ra = brank[c * BIAS_CHUNK], rb = brank[kb - 1];
        sbase[c] = (int32_t)(nslots - ra);
        nslots += rb - ra + 1;
        if (ra < nsr) {
            npts3 += kb - c * BIAS_CHUNK;
            nslots3 += rb - ra + 1;
        }
    }
    std::vector<int32_t> long_rank, long_of(std::max<int64_t>(ns, 1), -1);
    for (int64_t r = 0; r < ns; ++r)
        if ((seg[r + 1] - 1) / BIAS_CHUNK - seg[r] / BIAS_CHUNK + 1 > BIAS_LONG) {
            long_of[r] = (int32_t)long_rank.size();
            long_rank.push_back((int32_t)r);
        }
    BiasData& B = S.bias;
    B.nb = nb; B.ns = ns; B.npts = npts; B.nchunk = nchunk; B.nslots = nslots;
    B.nlong = (int64_t)long_rank.size();
    const int nch = h_grp ? 3 : 1;
    B.lsum.alloc(std::max<int64_t>(B.nlong, 1) * nch);
    B.nbk = grid_for(ns, BLOCK, BIAS_NPART);
    auto up = [&](DBuf<int32_t>& d, const std::vector<int32_t>& h) {
        d.alloc((int64_t)h.size());
        d.upload(h.data(), (int64_t)h.size(), S.stream);
    };
    auto upd = [&](DBuf<double>& d, const std::vector<double>& h) {
        d.alloc((int64_t)h.size());
        d.upload(h.data(), (int64_t)h.size(), S.stream);
    };
    up(B.idx, idx); up(B.brank, brank); up(B.rank_pt, rank_pt); up(B.seg, seg); up(B.sbase, sbase);
    up(B.long_of, long_of);
    long_rank.resize(std::max<size_t>(long_rank.size(), 1));
    up(B.long_rank, long_rank);
    rank_id.resize(std::max<int64_t>(ns, 1));
    up(B.rank_id, rank_id);
    upd(B.c2, c2);
    B.w2.alloc(std::max<int64_t>(npts, 1));
    B.D.alloc(std::max<int64_t>(ns, 1));
    B.sD.alloc(std::max<int64_t>(ns, 1));
    B.slots.alloc(std::max<int64_t>(nslots, 1) * nch);
    B.bval.alloc(nb + 1);   // the sink's rank scatters its 0 behind the IDs
    std::vector<double> u, gc2;
    if (h_grp) {
        B.ng = ng; B.nsr = nsr; B.npts3 = npts3; B.nslots3 = nslots3; B.pseudo = pseudo;
        B.nrk = grid_for(ns, BLOCK, BIAS_NPART / 2);
        B.ngk = grid_for(ng, BLOCK / 64, BIAS_NPART / 2);
        B.nbk = B.nrk + B.ngk;
        u.assign(2 * std::max<int64_t>(npts, 1), 0.0);
        for (int64_t i = 0; i < npts; ++i)
            if (h_grp[perm[i]] >= 0 && !sunk(perm[i])) {
                u[2 * i] = h_u[2 * (int64_t)perm[i]];
                u[2 * i + 1] = h_u[2 * (int64_t)perm[i] + 1];
            }
        gc2.resize(2 * ng);
        for (int64_t k = 0; k < 2 * ng; ++k) gc2[k] = h_gc[k] * h_gc[k];
        rgrp.resize(std::max<int64_t>(nsr, 1));
        up(B.gseg, gseg); up(B.rgrp, rgrp);
        upd(B.u, u); upd(B.gc2, gc2);
        B.rsum.alloc(3 * std::max<int64_t>(ns, 1));
        B.e.alloc(2 * std::max<int64_t>(ns, 1));
        B.F.alloc(3 * ng); B.L.alloc(3 * ng); B.gam.alloc(2 * ng); B.gval.alloc(2 * ng);
        B.tmp.alloc(std::max<int64_t>(npts, 1));
    }
    HIP_CHECK(hipStreamSynchronize(S.stream));   // the uploads read host vectors of this scope
    B.h_id = std::move(keep_id);
    B.h_c = std::move(keep_c);
    B.h_grp = std::move(keep_grp);
    B.h_u = std::move(keep_u);
    B.h_gc = std::move(keep_gc);
    B.h_sink = std::move(keep_sink);
    B.sink = has_sink;
    B.on = npts > 0 && ns > 0;   // no data rows: every bias is 0, the operator is unchanged
}
}  // namespace

// id: the data rows' bias IDs in the caller's row order; c: 1 / E_bias per ID.  Clears the slopes.
void bias_set(System& S, int64_t npts, const int32_t* h_id, int64_t nb, const double* h_c) {
    if (!S.mf || S.dist) throw std::invalid_argument("lsq_set_data_bias: needs a single-GPU structured system (lsq_set_matrix_stencil)");
    if (S.sgrid.ng) throw std::invalid_argument("lsq_set_data_bias: sensor grids are set (lsq_set_sensor_grids); clear them first");
    if (npts != S.mfh.npts) throw std::invalid_argument("lsq_set_data_bias: npts differs from the system's data rows");
    if (nb >= (int64_t)INT32_MAX) throw std::invalid_argument("lsq_set_data_bias: too many bias IDs");
    if (!S.dmf.ok || S.dmf.npts != npts)
        throw std::invalid_argument("lsq_set_data_bias: needs matrix-free data rows (interpolation grids on one (y, x) lattice)");
    // validation on the device
    DBuf<int32_t> did(std::max<int64_t>(npts, 1));
    DBuf<double> dc(nb);
    DBuf<int> flag(1);
    did.upload(h_id, npts, S.stream);
    dc.upload(h_c, nb, S.stream);
    flag.zero(S.stream);
    hipLaunchKernelGGL(k_bias_validate, dim3(grid_for(std::max(npts, nb))), dim3(BLOCK), 0, S.stream, npts, did.p, nb,
                       dc.p, flag.p);
    KERNEL_CHECK();
    int hf = 0;
    flag.download(&hf, 1, S.stream);
    HIP_CHECK(hipStreamSynchronize(S.stream));
    if (hf & 1) throw std::invalid_argument("lsq_set_data_bias: a bias ID lies outside [0, nb)");
    if (hf & 2) throw std::invalid_argument("lsq_set_data_bias: every c must be > 0");
    bias_build(S, npts, h_id, nb, h_c, nullptr, nullptr, 0, nullptr);
}

// the slopes cleared: the bias-only layout again (bit for bit the one lsq_set_data_bias made), or nothing
void slope_clear(System& S) {
    if (!S.bias.ng) return;
    if (!S.bias.nb) {
        bias_clear(S);
        return;
    }
    const std::vector<int32_t> id = S.bias.h_id;
    const std::vector<double> c = S.bias.h_c;
    bias_build(S, (int64_t)id.size(), id.data(), (int64_t)c.size(), c.data(), nullptr, nullptr, 0, nullptr);
}

// grp: the data rows' slope groups (−1: none) in the caller's row order, u: two coefficients per row,
// c: two constraint weights per group
void slope_set(System& S, int64_t npts, const int32_t* h_grp, const double* h_u, int64_t ng, const double* h_c) {
    if (!S.mf || S.dist) throw std::invalid_argument("lsq_set_data_slope: needs a single-GPU structured system (lsq_set_matrix_stencil)");
    if (S.sgrid.ng) throw std::invalid_argument("lsq_set_data_slope: sensor grids are set (lsq_set_sensor_grids); clear them first");
    if (npts != S.mfh.npts) throw std::invalid_argument("lsq_set_data_slope: npts differs from the system's data rows");
    if (ng >= (int64_t)INT32_MAX - 1) throw std::invalid_argument("lsq_set_data_slope: too many slope groups");
    if (!S.dmf.ok || S.dmf.npts != npts)
        throw std::invalid_argument("lsq_set_data_slope: needs matrix-free data rows (interpolation grids on one (y, x) lattice)");
    for (int64_t k = 0; k < 2 * ng; ++k)
        if (!(h_c[k] > 0.0)) throw std::invalid_argument("lsq_set_data_slope: every c must be > 0");
    const int64_t nb = S.bias.nb;
    std::vector<int32_t> sgrp(nb, -1);   // nested: the rows of a bias ID lie in at most one group
    for (int64_t i = 0; i < npts; ++i) {
        const int32_t g = h_grp[i];
        if (g < -1 || g >= ng) throw std::invalid_argument("lsq_set_data_slope: a slope group lies outside {-1} and [0, ng)");
        if (g < 0) continue;
        if (!std::isfinite(h_u[2 * i]) || !std::isfinite(h_u[2 * i + 1]))
            throw std::invalid_argument("lsq_set_data_slope: a coefficient u is not finite");
        if (nb) {
            int32_t& sg = sgrp[S.bias.h_id[i]];
            if (sg >= 0 && sg != g)
                throw std::invalid_argument("lsq_set_data_slope: the layout is not nested (the rows of a bias ID lie in "
                                            "more than one slope group)");
            sg = g;
        }
    }
    if (nb) {
        const std::vector<int32_t> id = S.bias.h_id;
        const std::vector<double> c = S.bias.h_c;
        bias_build(S, npts, id.data(), nb, c.data(), h_grp, h_u, ng, h_c);
    } else {
        bias_build(S, npts, nullptr, 0, nullptr, h_grp, h_u, ng, h_c);
    }
}

// the biases (and slopes) of the x in S.cg_x (full space) for the right-hand side dbp:
// [b; γ] = M⁻¹ Zᵀ W² (d − A_d x); without slopes b_j = Σ W²(d − A_d x) / D_j
void bias_values(System& S, const double* dbp) {
    BiasData& B = S.bias;
    B.bval.zero(S.stream);
    if (B.ng) B.gval.zero(S.stream);
    if (bias_active(S)) {
        const CgGrids g = cg_grids(S, 1);
        DBuf<CgState> st(1);
        st.zero(S.stream);
        hipLaunchKernelGGL(k_cg_dmf_ad, dim3(g.gD), dim3(BLOCK), 0, S.stream, st.p, S.dmf,
                           reinterpret_cast<const double4*>(S.dmf_pt.p), S.cg_x.p, S.cg_t.p, S.cg_part_t.p);
        hipLaunchKernelGGL(k_bias_resid, dim3(grid_for(B.npts)), dim3(BLOCK), 0, S.stream, B.npts, S.dmf_perm.p, B.w2.p,
                           dbp, S.cg_t.p, S.cg_t.p);
        bias_launch_reduce(S, nullptr, S.cg_t.p, nullptr);
        if (!B.pseudo)
            hipLaunchKernelGGL(k_bias_scatter, dim3(grid_for(B.ns)), dim3(BLOCK), 0, S.stream, B.ns, B.rank_id.p, B.sD.p,
                               B.bval.p);
        if (B.ng)
            HIP_CHECK(hipMemcpyAsync(B.gval.p, B.gam.p, 2 * B.ng * sizeof(double), hipMemcpyDeviceToDevice, S.stream));
        KERNEL_CHECK();
        HIP_CHECK(hipStreamSynchronize(S.stream));
    }
    B.solved = true;
    B.gsolved = B.ng > 0;
}

void bias_get(System& S, double* h_b) {
    if (!S.bias.nb) throw std::invalid_argument("lsq_get_data_bias: no biases set");
    if (!S.bias.solved) throw std::invalid_argument("lsq_get_data_bias: no lsq_solve since the biases were set");
    S.bias.bval.download(h_b, S.bias.nb, S.stream);
    HIP_CHECK(hipStreamSynchronize(S.stream));
}

void slope_get(System& S, double* h_g) {
    if (!S.bias.ng) throw std::invalid_argument("lsq_get_data_slope: no slopes set");
    if (!S.bias.gsolved) throw std::invalid_argument("lsq_get_data_slope: no lsq_solve since the slopes were set");
    S.bias.gval.download(h_g, 2 * S.bias.ng, S.stream);
    HIP_CHECK(hipStreamSynchronize(S.stream));
}

// the layout of the biases and slopes that are set, built again with the rows of h_sink (null: none)
// taken out: without a sink bit for bit the layout lsq_set_data_bias / lsq_set_data_slope made
static void bias_rebuild(System& S, const uint8_t* h_sink) {
    const BiasData& B = S.bias;
    const std::vector<int32_t> id = B.h_id, grp = B.h_grp;
    const std::vector<double> c = B.h_c, u = B.h_u, gc = B.h_gc;
    const int64_t nb = B.nb, ng = B.ng, npts = (int64_t)(nb ? id.size() : grp.size());
    bias_build(S, npts, nb ? id.data() : nullptr, nb, nb ? c.data() : nullptr, ng ? grp.data() : nullptr,
               ng ? u.data() : nullptr, ng, ng ? gc.data() : nullptr, h_sink);
}

// ---- sensor bias grids (sgrid.inc): set, clear, read back ----------------------------------------
void sgrid_clear(System& S) {
    if (!S.sgrid.ng) return;
    graph_cache_drop(&S);   // captured iterations hold the step's launches
    S.sgrid = SgridData{};
    S.cg_ready = false;
    if (S.bias.sink) bias_rebuild(S, nullptr);   // the grids' rows return to the bias / slope path
}

// grid: the data rows' grids (−1: none) in the caller's row order; node, wt: four local nodes and
// weights per row; n_nodes per grid; K_s as triplets k_ptr[s] … k_ptr[s + 1] with local rows and columns.
// Every check runs before anything of the handle changes.
//
// joint (lsq_set_sensor_grids_joint): biases and slopes may be set.  A bias ID or a slope group with a
// row in a grid must have all its rows in that grid ("nested") and becomes a dense node of the grid's
// block (SgridData); the rows of every grid leave the bias / slope path (BiasData::sink).
void sgrid_set(System& S, int64_t npts, const int32_t* h_grid, const int32_t* h_node, const double* h_wt, int64_t ng,
               const int64_t* h_nn, const int64_t* k_ptr, const int32_t* k_row, const int32_t* k_col,
               const double* k_val, bool joint) {
    if (!S.mf || S.dist) throw std::invalid_argument("lsq_set_sensor_grids: needs a single-GPU structured system (lsq_set_matrix_stencil)");
    if (!joint && (S.bias.nb || S.bias.ng)) throw std::invalid_argument("lsq_set_sensor_grids: data biases or slopes are set; the joint block is not one matrix per grid");
    if (npts != S.mfh.npts) throw std::invalid_argument("lsq_set_sensor_grids: npts differs from the system's data rows");
    if (!S.dmf.ok || S.dmf.npts != npts)
        throw std::invalid_argument("lsq_set_sensor_grids: needs matrix-free data rows (interpolation grids on one (y, x) lattice)");
    std::vector<int64_t> nl(h_nn, h_nn + ng), nx(ng, 0), npad(ng), poff(ng + 1, 0), moff(ng + 1, 0);
    for (int64_t g = 0; g < ng; ++g)
        if (nl[g] < 1 || nl[g] > SG_MAX_NODES)
            throw std::invalid_argument("lsq_set_sensor_grids: grid " + std::to_string(g) + " has " + std::to_string(nl[g]) +
                                        " nodes; a grid holds 1 … " + std::to_string(SG_MAX_NODES) + " (the size cap)");
    // the dense nodes: the bias IDs (in ID order), then the slope groups (two nodes each) of every grid
    const bool jb = joint && S.bias.nb > 0, js = joint && S.bias.ng > 0;
    const int64_t nb = jb ? S.bias.nb : 0, nsg = js ? S.bias.ng : 0;
    const std::vector<int32_t>& b_id = S.bias.h_id;
    const std::vector<int32_t>& b_grp = S.bias.h_grp;
    std::vector<int32_t> id_grid(nb, -2), grp_grid(nsg, -2);   // −2: no row seen, −1: rows outside every grid
    std::vector<int32_t> id_loc(nb, -1), grp_loc(nsg, -1);     // the local node of a claimed ID, of a claimed group's x slope
    if (jb || js) {
        auto claim = [&](int32_t& owner, int32_t g, const char* what) {
            if (owner == -2)
                owner = g;
            else if (owner != g)
                throw std::invalid_argument(std::string("lsq_set_sensor_grids_joint: the layout is not nested (the rows of a ") +
                                            what + " lie in a grid and outside it, or in two grids)");
        };
        for (int64_t i = 0; i < npts; ++i) {
            const int32_t g = h_grid[i];
            if (g < -1 || g >= ng) throw std::invalid_argument("lsq_set_sensor_grids: a grid lies outside {-1} and [0, ng)");
            if (jb) claim(id_grid[b_id[i]], g, "bias ID");
            if (js && b_grp[i] >= 0) claim(grp_grid[b_grp[i]], g, "slope group");
        }
        for (int64_t j = 0; j < nb; ++j)
            if (id_grid[j] >= 0) id_loc[j] = (int32_t)(nl[id_grid[j]] + nx[id_grid[j]]++);
        for (int64_t s = 0; s < nsg; ++s)
            if (grp_grid[s] >= 0) {
                grp_loc[s] = (int32_t)(nl[grp_grid[s]] + nx[grp_grid[s]]);
                nx[grp_grid[s]] += 2;
            }
    }
    std::vector<int64_t> nn(ng);
    int64_t nxt = 0;
    for (int64_t g = 0; g < ng; ++g) {
        if (nx[g] > SG_MAX_DENSE)
            throw std::invalid_argument("lsq_set_sensor_grids_joint: grid " + std::to_string(g) + " has " + std::to_string(nx[g]) +
                                        " dense nodes (bias IDs and slopes inside it); the cap is " + std::to_string(SG_MAX_DENSE));
        nn[g] = nl[g] + nx[g];
        nxt += nx[g];
        if (nn[g] > SG_MAX_NODES)
            throw std::invalid_argument("lsq_set_sensor_grids_joint: grid " + std::to_string(g) + " has " + std::to_string(nn[g]) +
                                        " lattice and dense nodes; a block holds 1 … " + std::to_string(SG_MAX_NODES) + " (the size cap)");
        npad[g] = (nn[g] + 63) / 64 * 64;
        poff[g + 1] = poff[g] + npad[g];
        moff[g + 1] = moff[g] + npad[g] * npad[g];
        if (moff[g + 1] * (int64_t)sizeof(double) > SG_MAX_FACTOR_BYTES)
            throw std::invalid_argument("lsq_set_sensor_grids: the grids' inverse factors exceed the size cap of " +
                                        std::to_string(SG_MAX_FACTOR_BYTES) + " bytes");
    }
    const int64_t ntp = poff[ng];
    if (k_ptr && k_ptr[0] != 0) throw std::invalid_argument("lsq_set_sensor_grids: k_ptr must start at 0");
    std::vector<std::pair<int64_t, double>> kent;   // (position, value), input order
    for (int64_t g = 0; g < ng && k_ptr; ++g) {
        if (k_ptr[g + 1] < k_ptr[g]) throw std::invalid_argument("lsq_set_sensor_grids: k_ptr must not decrease");
        for (int64_t t = k_ptr[g]; t < k_ptr[g + 1]; ++t) {
            if (k_row[t] < 0 || k_row[t] >= nl[g] || k_col[t] < 0 || k_col[t] >= nl[g])
                throw std::invalid_argument("lsq_set_sensor_grids: an entry of K lies outside its grid's nodes");
            if (!std::isfinite(k_val[t])) throw std::invalid_argument("lsq_set_sensor_grids: a value of K is not finite");
            kent.emplace_back(moff[g] + (int64_t)k_row[t] * npad[g] + k_col[t], k_val[t]);
        }
    }
    for (int64_t i = 0; i < npts; ++i) {
        const int32_t g = h_grid[i];
        if (g < -1 || g >= ng) throw std::invalid_argument("lsq_set_sensor_grids: a grid lies outside {-1} and [0, ng)");
        if (g < 0) continue;
        for (int q = 0; q < 4; ++q) {
            if (h_node[4 * i + q] < 0 || h_node[4 * i + q] >= nl[g])
                throw std::invalid_argument("lsq_set_sensor_grids: a node lies outside its grid");
            if (!std::isfinite(h_wt[4 * i + q])) throw std::invalid_argument("lsq_set_sensor_grids: a weight is not finite");
        }
    }
    std::vector<int32_t> perm(std::max<int64_t>(npts, 1));
    S.dmf_perm.download(perm.data(), npts, S.stream);
    HIP_CHECK(hipStreamSynchronize(S.stream));
    // the dense nodes' c² on the diagonal, behind K's entries
    std::vector<int32_t> cl_id, cl_id_node, cl_grp, cl_grp_node;
    for (int64_t j = 0; j < nb; ++j)
        if (id_loc[j] >= 0) {
            const int64_t g = id_grid[j], d = id_loc[j];
            kent.emplace_back(moff[g] + d * npad[g] + d, S.bias.h_c[j] * S.bias.h_c[j]);
            cl_id.push_back((int32_t)j);
            cl_id_node.push_back((int32_t)(poff[g] + d));
        }
    for (int64_t s = 0; s < nsg; ++s)
        if (grp_loc[s] >= 0) {
            const int64_t g = grp_grid[s];
            for (int64_t k = 0; k < 2; ++k) {
                const int64_t d = grp_loc[s] + k;
                kent.emplace_back(moff[g] + d * npad[g] + d, S.bias.h_gc[2 * s + k] * S.bias.h_gc[2 * s + k]);
            }
            cl_grp.push_back((int32_t)s);
            cl_grp_node.push_back((int32_t)(poff[g] + grp_loc[s]));
        }
    // the rows that lie in a grid, in sorted point order; the transpose by padded node in that order
    std::vector<int32_t> gp_pt, gp_node, gp_xnode;
    std::vector<double> gp_wt, gp_xu;
    std::vector<int64_t> tr_ptr(ntp + 1, 0);
    for (int64_t i = 0; i < npts; ++i) {
        const int64_t r = perm[i];
        const int32_t g = h_grid[r];
        if (g < 0) continue;
        gp_pt.push_back((int32_t)i);
        for (int q = 0; q < 4; ++q) {
            const int32_t k = (int32_t)(poff[g] + h_node[4 * r + q]);
            gp_node.push_back(k);
            gp_wt.push_back(h_wt[4 * r + q]);
            if (h_wt[4 * r + q] != 0.0) ++tr_ptr[k + 1];
        }
        if (!nxt) continue;
        // the row's dense entries: its ID's node, its group's two (every ID and group of a grid's row is claimed by the grid)
        const int32_t kb = jb ? (int32_t)(poff[g] + id_loc[b_id[r]]) : -1;
        const int32_t ks = js && b_grp[r] >= 0 ? (int32_t)(poff[g] + grp_loc[b_grp[r]]) : -1;
        gp_xnode.insert(gp_xnode.end(), {kb, ks, ks >= 0 ? ks + 1 : -1, -1});
        gp_xu.push_back(ks >= 0 ? S.bias.h_u[2 * r] : 0.0);
        gp_xu.push_back(ks >= 0 ? S.bias.h_u[2 * r + 1] : 0.0);
        if (kb >= 0) ++tr_ptr[kb + 1];
        if (ks >= 0) {
            ++tr_ptr[ks + 1];
            ++tr_ptr[ks + 2];
        }
    }
    const int64_t ngp = (int64_t)gp_pt.size();
    for (int64_t k = 0; k < ntp; ++k) tr_ptr[k + 1] += tr_ptr[k];
    const int64_t nent = tr_ptr[ntp];
    if (nent >= (int64_t)INT32_MAX) throw std::invalid_argument("lsq_set_sensor_grids: too many entries");
    // the dense nodes' long lists in segments of SG_SEG entries (k_sg_btd_seg)
    std::vector<int32_t> seg_ptr(ntp + 1, 0);
    std::vector<int64_t> seg_lo, seg_hi;
    // LSQ_SG_SEG=0 (read at set time): one wave per list, the layout tools/sgrid_joint_step.py measures against
    const bool seg_on = !getenv("LSQ_SG_SEG") || atoi(getenv("LSQ_SG_SEG")) != 0;
    for (int64_t g = 0; g < ng && nxt && seg_on; ++g)
        for (int64_t d = nl[g]; d < nn[g]; ++d) {
            const int64_t k = poff[g] + d;
            if (tr_ptr[k + 1] - tr_ptr[k] <= SG_SEG) continue;
            for (int64_t lo = tr_ptr[k]; lo < tr_ptr[k + 1]; lo += SG_SEG) {
                seg_lo.push_back(lo);
                seg_hi.push_back(std::min(lo + SG_SEG, tr_ptr[k + 1]));
                ++seg_ptr[k + 1];
            }
        }
    for (int64_t k = 0; k < ntp; ++k) seg_ptr[k + 1] += seg_ptr[k];
    const int64_t nseg = (int64_t)seg_lo.size();
    std::vector<int32_t> tr_pt(std::max<int64_t>(nent, 1)), tr_gp(std::max<int64_t>(nent, 1)), nbr(std::max<int64_t>(ntp, 1) * SG_NBR, -1);
    std::vector<uint32_t> tr_slot(std::max<int64_t>(nent, 1));
    std::vector<double> tr_w(std::max<int64_t>(nent, 1));
    std::vector<int64_t> fill(tr_ptr.begin(), tr_ptr.end() - 1);
    for (int64_t j = 0; j < ngp && nxt; ++j)   // the dense nodes' lists: every row of the ID or group, in point order
        for (int q = 0; q < 3; ++q) {
            const int32_t k = gp_xnode[4 * j + q];
            if (k < 0) continue;
            const int64_t e = fill[k]++;
            tr_pt[e] = gp_pt[j];
            tr_gp[e] = (int32_t)j;
            tr_w[e] = q == 0 ? 1.0 : gp_xu[2 * j + q - 1];
            tr_slot[e] = 0xffffffffu;   // k_sg_asm does not walk these lists
        }
    for (int64_t j = 0; j < ngp; ++j)
        for (int q0 = 0; q0 < 4; ++q0) {
            if (gp_wt[4 * j + q0] == 0.0) continue;
            const int32_t k = gp_node[4 * j + q0];
            const int64_t e = fill[k]++;
            tr_pt[e] = gp_pt[j];
            tr_gp[e] = (int32_t)j;
            tr_w[e] = gp_wt[4 * j + q0];
            uint32_t sl = 0;
            for (int q = 0; q < 4; ++q) {
                uint32_t slot = 255;
                if (gp_wt[4 * j + q] != 0.0) {
                    int32_t* nb = nbr.data() + (int64_t)k * SG_NBR;
                    int c = 0;
                    while (c < SG_NBR && nb[c] >= 0 && nb[c] != gp_node[4 * j + q]) ++c;
                    if (c == SG_NBR)
                        throw std::invalid_argument("lsq_set_sensor_grids: a node shares rows with more than 9 nodes "
                                                    "(the rows must be cells of a lattice)");
                    nb[c] = gp_node[4 * j + q];
                    slot = (uint32_t)c;
                }
                sl |= slot << (8 * q);
            }
            tr_slot[e] = sl;
        }
    // K: duplicates summed in input order
    std::stable_sort(kent.begin(), kent.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    std::vector<int64_t> k_pos;
    std::vector<double> k_sum;
    for (const auto& kv : kent) {
        if (!k_pos.empty() && k_pos.back() == kv.first)
            k_sum.back() += kv.second;
        else {
            k_pos.push_back(kv.first);
            k_sum.push_back(kv.second);
        }
    }
    std::vector<int32_t> node_grid(std::max<int64_t>(ntp, 1), 0), tile_grid, tile_jb;
    for (int64_t g = 0; g < ng; ++g) {
        for (int64_t k = poff[g]; k < poff[g + 1]; ++k) node_grid[k] = (int32_t)g;
        for (int64_t jb = 0; jb < npad[g] / 64; ++jb) {
            tile_grid.push_back((int32_t)g);
            tile_jb.push_back((int32_t)jb);
        }
    }
    // device memory first: a failed allocation leaves the handle as it was
    SgridData N;
    N.ng = ng; N.npts = npts; N.ntp = ntp; N.ngp = ngp; N.nent = nent;
    N.ntile = (int64_t)tile_grid.size(); N.nk = (int64_t)k_pos.size(); N.fsum = moff[ng];
    for (int64_t g = 0; g < ng; ++g) N.ntot += nl[g];
    N.nbk = grid_for(ntp, BLOCK, BIAS_NPART);
    N.h_nn = nn; N.h_nl = nl; N.h_npad = npad; N.h_poff = poff; N.h_moff = moff;
    N.nxt = nxt;
    N.cl_id = cl_id; N.cl_id_node = cl_id_node; N.cl_grp = cl_grp; N.cl_grp_node = cl_grp_node;
    auto up = [&](auto& d, const auto& h) {
        d.alloc(std::max<int64_t>((int64_t)h.size(), 1));
        d.upload(h.data(), (int64_t)h.size(), S.stream);
    };
    gp_pt.resize(std::max<int64_t>(ngp, 1));
    gp_node.resize(4 * std::max<int64_t>(ngp, 1));
    gp_wt.resize(4 * std::max<int64_t>(ngp, 1));
    up(N.tr_ptr, tr_ptr); up(N.tr_pt, tr_pt); up(N.tr_gp, tr_gp); up(N.tr_slot, tr_slot); up(N.tr_w, tr_w);
    up(N.gp_pt, gp_pt); up(N.gp_node, gp_node); up(N.gp_wt, gp_wt); up(N.nbr, nbr); up(N.node_grid, node_grid);
    up(N.poff, poff); up(N.moff, moff); up(N.npad, npad); up(N.nn, nn); up(N.tile_grid, tile_grid); up(N.tile_jb, tile_jb);
    up(N.k_pos, k_pos); up(N.k_val, k_sum);
    up(N.nl, nl); up(N.nx, nx);
    if (nxt) {
        up(N.gp_xnode, gp_xnode); up(N.gp_xu, gp_xu);
    }
    N.nseg = nseg;
    if (nseg) {
        up(N.seg_ptr, seg_ptr); up(N.seg_lo, seg_lo); up(N.seg_hi, seg_hi);
        N.seg_sum.alloc(nseg);
    }
    N.w2.alloc(std::max<int64_t>(npts, 1));
    N.M.alloc(N.fsum); N.Ri.alloc(N.fsum);
    N.d0.alloc(ntp); N.err.alloc(ng);
    N.s.alloc(ntp); N.z.alloc(ntp); N.y.alloc(ntp);
    N.aval.assign(N.ntot, 0.0);
    HIP_CHECK(hipStreamSynchronize(S.stream));   // the uploads read host vectors of this scope
    N.on = npts > 0;
    graph_cache_drop(&S);   // captured iterations hold no elimination step yet
    if (jb || js) {   // the grids' rows leave the bias / slope path
        std::vector<uint8_t> sink(std::max<int64_t>(npts, 1), 0);
        for (int64_t i = 0; i < npts; ++i) sink[i] = h_grid[i] >= 0;
        bias_rebuild(S, sink.data());
    }
    S.sgrid = std::move(N);
    S.cg_ready = false;
}

// the grids of the x in S.cg_x (full space) for the right-hand side dbp: a = M⁻¹ Bᵀ W² (d − A_d x)
void sgrid_values(System& S, const double* dbp) {
    SgridData& G = S.sgrid;
    std::fill(G.aval.begin(), G.aval.end(), 0.0);
    if (sgrid_active(S)) {
        const CgGrids g = cg_grids(S, 1);
        DBuf<CgState> st(1);
        st.zero(S.stream);
        hipLaunchKernelGGL(k_cg_dmf_ad, dim3(g.gD), dim3(BLOCK), 0, S.stream, st.p, S.dmf,
                           reinterpret_cast<const double4*>(S.dmf_pt.p), S.cg_x.p, S.cg_t.p, S.cg_part_t.p);
        hipLaunchKernelGGL(k_bias_resid, dim3(grid_for(G.npts)), dim3(BLOCK), 0, S.stream, G.npts, S.dmf_perm.p, G.w2.p,
                           dbp, S.cg_t.p, S.cg_t.p);
        sgrid_launch_reduce(S, nullptr, S.cg_t.p);
        KERNEL_CHECK();
        std::vector<double> y(G.ntp);
        G.y.download(y.data(), G.ntp, S.stream);
        HIP_CHECK(hipStreamSynchronize(S.stream));
        int64_t o = 0;
        for (int64_t s = 0; s < G.ng; ++s)
            for (int64_t k = 0; k < G.h_nl[s]; ++k) G.aval[o++] = y[G.h_poff[s] + k];
        // the claimed biases and slopes are their blocks' dense nodes (bias_values ran before and left them 0)
        // (the biases and slopes cannot change while grids are set: api.hip refuses their set and clear calls)
        BiasData& B = S.bias;
        if ((!G.cl_id.empty() && G.cl_id.back() >= B.nb) || (!G.cl_grp.empty() && G.cl_grp.back() >= B.ng))
            throw std::logic_error("sensor grids: the claimed biases or slopes left the handle");
        if (!G.cl_id.empty()) {
            std::vector<double> b(B.nb);
            B.bval.download(b.data(), B.nb, S.stream);
            HIP_CHECK(hipStreamSynchronize(S.stream));
            for (size_t t = 0; t < G.cl_id.size(); ++t) b[G.cl_id[t]] = y[G.cl_id_node[t]];
            B.bval.upload(b.data(), B.nb, S.stream);
            HIP_CHECK(hipStreamSynchronize(S.stream));
        }
        if (!G.cl_grp.empty()) {
            std::vector<double> gv(2 * B.ng);
            B.gval.download(gv.data(), 2 * B.ng, S.stream);
            HIP_CHECK(hipStreamSynchronize(S.stream));
            for (size_t t = 0; t < G.cl_grp.size(); ++t) {
                gv[2 * G.cl_grp[t]] = y[G.cl_grp_node[t]];
                gv[2 * G.cl_grp[t] + 1] = y[G.cl_grp_node[t] + 1];
            }
            B.gval.upload(gv.data(), 2 * B.ng, S.stream);
            HIP_CHECK(hipStreamSynchronize(S.stream));
        }
    }
    G.solved = true;
}

void sgrid_get(System& S, double* h_a) {
    if (!S.sgrid.ng) throw std::invalid_argument("lsq_get_sensor_grids: no sensor grids set");
    if (!S.sgrid.solved) throw std::invalid_argument("lsq_get_sensor_grids: no lsq_solve since the grids were set");
    std::copy(S.sgrid.aval.begin(), S.sgrid.aval.end(), h_a);
}

// why a solve with biases, slopes or sensor grids set cannot run (empty: it can)
std::string bias_refusal(System& S, int method, int precond) {
    if (!S.bias.nb && !S.bias.ng && !S.sgrid.ng) return "";
    const std::string what = S.sgrid.ng ? "sensor grids" : (S.bias.nb ? "data biases" : "data slopes");
    if (S.dist) return what + " run on single-GPU handles only";
    if (method != 1) return what + " need CGNR (method 1)";
    if (precond != 1 && precond != 3 && precond != 4) return what + " run with precond 1, 3 or 4";
    if (!cg_available(S, precond)) return what + " need the structured CGNR operator: " + (S.cg_ok ? S.mg_why : S.cg_why);
    if (!cg_use_dmf(S)) return what + " need the matrix-free column-mode CGNR data rows (tile mode is not covered)";
    return "";
}

// ---- extra rows (xrows.inc): formation, column norms, refusals ----------------------------------
// The staged rows (merged, zero-free, columns ascending, full ids, no removed column: api.hip) on
// the device: SELL-64 slices, the transpose over the touched columns, and the CSR over the compact
// columns that ensure_full_csr appends to G.  row0: the system row of the first extra row.
void xr_form(System& S, int64_t row0) {
    XrData& X = S.xr;
    const int64_t m_x = X.st_m, nf = S.mfh.n_full;
    const int64_t nnz = m_x ? X.st_rp[m_x] : 0;
    for (int64_t e = 0; e < nnz; ++e)
        if (X.st_ci[e] < 0 || X.st_ci[e] >= nf)
            throw std::invalid_argument("lsq_set_matrix_stencil: an extra row's column lies outside [0, n_full)");
    X.m_x = m_x;
    X.row0 = row0;
    X.nnz = nnz;
    X.on = false;
    X.lump_req = m_x > 0 && X.st_lump;   // the tables follow with the hierarchy (mg.inc, xr_lump_prepare)
    X.lump_built = X.lump_ok = false;
    X.lump_why.clear();
    X.l_rows = X.l_nodes = X.l_ent = X.l_long = X.l_dev_bytes = 0;
    if (!m_x) return;
    std::vector<int32_t> cmap;
    if (S.have_colmap) {
        cmap.resize(nf);
        S.colmap.download(cmap.data(), nf, S.stream);
        HIP_CHECK(hipStreamSynchronize(S.stream));
    }
    X.h_rp.assign(X.st_rp.begin(), X.st_rp.end());
    X.h_ci.resize(nnz);
    X.h_val.assign(X.st_val.begin(), X.st_val.end());
    for (int64_t e = 0; e < nnz; ++e) X.h_ci[e] = S.have_colmap ? cmap[X.st_ci[e]] : (int32_t)X.st_ci[e];
    // SELL-64: a slice is as wide as its longest row; padding carries value 0 and column 0
    const int64_t nsl = (m_x + SELL_C - 1) / SELL_C;
    std::vector<int64_t> sp(nsl + 1, 0);
    for (int64_t s = 0; s < nsl; ++s) {
        int64_t w = 0;
        for (int64_t r = s * SELL_C; r < std::min(m_x, (s + 1) * SELL_C); ++r) w = std::max(w, X.st_rp[r + 1] - X.st_rp[r]);
        sp[s + 1] = sp[s] + w * SELL_C;
    }
    const int64_t nent = sp[nsl];
    std::vector<int32_t> sci(std::max<int64_t>(nent, 1), 0);
    std::vector<double> sval(std::max<int64_t>(nent, 1), 0.0);
    for (int64_t r = 0; r < m_x; ++r) {
        const int64_t base = sp[r / SELL_C] + r % SELL_C;
        for (int64_t e = X.st_rp[r]; e < X.st_rp[r + 1]; ++e) {
            sci[base + (e - X.st_rp[r]) * SELL_C] = (int32_t)X.st_ci[e];
            sval[base + (e - X.st_rp[r]) * SELL_C] = X.st_val[e];
        }
    }
    // transpose over the touched columns: rows ascending inside a column (the rows are walked in order)
    std::vector<int32_t> tc(X.st_ci.begin(), X.st_ci.end());
    std::sort(tc.begin(), tc.end());
    tc.erase(std::unique(tc.begin(), tc.end()), tc.end());
    const int64_t ntc = (int64_t)tc.size();
    std::vector<int64_t> cp(ntc + 1, 0);
    std::vector<int32_t> where(std::max<int64_t>(nnz, 1));
    for (int64_t e = 0; e < nnz; ++e) {
        where[e] = (int32_t)(std::lower_bound(tc.begin(), tc.end(), (int32_t)X.st_ci[e]) - tc.begin());
        ++cp[where[e] + 1];
    }
    for (int64_t j = 0; j < ntc; ++j) cp[j + 1] += cp[j];
    std::vector<int64_t> fill(cp.begin(), cp.end() - 1);
    std::vector<int32_t> cr(std::max<int64_t>(nnz, 1), 0), long_col;
    std::vector<double> cv(std::max<int64_t>(nnz, 1), 0.0);
    for (int64_t r = 0; r < m_x; ++r)
        for (int64_t e = X.st_rp[r]; e < X.st_rp[r + 1]; ++e) {
            const int64_t k = fill[where[e]]++;
            cr[k] = (int32_t)r;
            cv[k] = X.st_val[e];
        }
    for (int64_t j = 0; j < ntc; ++j)
        if (cp[j + 1] - cp[j] > XR_LONG) long_col.push_back((int32_t)j);
    X.ntc = ntc;
    X.nlong = (int64_t)long_col.size();
    X.nbk = grid_for(nsl, BLOCK / 64, XR_NPART);
    hipStream_t st = S.stream;
    X.rows.rows = m_x;
    X.rows.nslices = nsl;
    X.rows.nent = nent;
    X.rows.sp.alloc(nsl + 1);
    X.rows.sp.upload(sp.data(), nsl + 1, st);
    X.rows.ci.alloc((int64_t)sci.size());
    X.rows.ci.upload(sci.data(), (int64_t)sci.size(), st);
    X.rows.val.alloc((int64_t)sval.size());
    X.rows.val.upload(sval.data(), (int64_t)sval.size(), st);
    tc.resize(std::max<int64_t>(ntc, 1), 0);
    X.tc.alloc((int64_t)tc.size());
    X.tc.upload(tc.data(), (int64_t)tc.size(), st);
    X.cp.alloc(ntc + 1);
    X.cp.upload(cp.data(), ntc + 1, st);
    X.cr.alloc((int64_t)cr.size());
    X.cr.upload(cr.data(), (int64_t)cr.size(), st);
    X.cv.alloc((int64_t)cv.size());
    X.cv.upload(cv.data(), (int64_t)cv.size(), st);
    long_col.resize(std::max<size_t>(long_col.size(), 1), 0);
    X.long_col.alloc((int64_t)long_col.size());
    X.long_col.upload(long_col.data(), (int64_t)long_col.size(), st);
    X.tblk.alloc(std::max<int64_t>(ntc, 1));
    X.t.alloc(m_x);
    X.t.zero(st);
    HIP_CHECK(hipStreamSynchronize(st));
    X.dev_bytes = (int64_t)(X.rows.sp.bytes() + X.rows.ci.bytes() + X.rows.val.bytes() + X.tc.bytes() + X.cp.bytes() +
                            X.cr.bytes() + X.cv.bytes() + X.long_col.bytes() + X.tblk.bytes() + X.t.bytes());
    // rows that kept no entry still carry b: ‖W_x b_x‖² belongs to ‖b‖ and ‖r0‖ as LSQR on the full
    // CSR counts it, so they stay on (the kernels then walk empty slices and no touched column)
    X.on = true;
}

// norm2 (full space) += the extra rows' squared column norms for the current row scale
void xr_add_colnorm(System& S, double* norm2_full) {
    const XrData& X = S.xr;
    hipLaunchKernelGGL(k_xr_colnorm, dim3(grid_for(X.ntc)), dim3(BLOCK), 0, S.stream, X.ntc, X.tc.p, X.cp.p, X.cr.p,
                       X.cv.p, S.rs.p + X.row0, norm2_full);
    KERNEL_CHECK();
}

// why a solve with extra rows set cannot run (empty: it can)
std::string xr_refusal(System& S, int method, int precond, int op) {
    if (!S.xr.m_x) return "";
    if (S.dist) return "extra rows run on single-GPU handles only";
    if (method == 1 && precond == 4) {
        if (!S.xr.lump_req)
            return "multigrid (precond 4) does not carry extra rows: its coarse levels would miss their term";
        // lumping requested (lsq_set_extra_rows_lumping): the hierarchy carries them when every row fits
        // a node block and level 0 is the shared-lattice column-mode operator
        if (!cg_available(S, 4)) return "";   // the caller reports why there is no hierarchy
        if (S.mg->mixed)
            return "multigrid (precond 4) with lumped extra rows: the z0-refined hierarchy does not carry them";
        if (S.xr.on && !S.cgh.colmode)
            return "multigrid (precond 4) with lumped extra rows needs the column-mode CGNR operator";
        if (!S.xr.lump_ok)
            return "multigrid (precond 4): the extra rows cannot be lumped: " +
                   (S.xr.lump_why.empty() ? std::string("no tables for this hierarchy") : S.xr.lump_why);
        return "";
    }
    if (method == 1 && (precond == 1 || precond == 3) && cg_available(S, precond)) {
        if (S.xr.on && !S.cgh.colmode) return "extra rows need the column-mode CGNR operator";
        return "";
    }
    if (S.mf && op == 0 && precond != 2 && precond != 5)
        return "extra rows: LSQR runs on the assembled operator only (op = 1), not the structured stencil operator";
    return "";
}

// lsq_extra_rows_mg_info: {lumped rows, touched level-1 nodes, algorithmic bytes of one lumping
// pass, device bytes of its tables}; zeros when the rows are not lumped
void xr_mg_info(System& S, double* out4) {
    out4[0] = out4[1] = out4[2] = out4[3] = 0.0;
    if (!S.xr.m_x || !S.xr.lump_req || S.dist) return;
    if (!cg_available(S, 4) || !S.mg || !S.xr.lump_ok) return;
    out4[0] = (double)S.xr.l_rows;
    out4[1] = (double)S.xr.l_nodes;
    out4[2] = xr_lump_bytes(S);
    out4[3] = (double)S.xr.l_dev_bytes;
}

// xr_step_bytes and the device bytes of the extra rows (lsq_extra_rows_info)
void xr_info(System& S, double* out4) {
    out4[0] = (double)S.xr.m_x;
    out4[1] = (double)S.xr.ntc;
    out4[2] = S.xr.on ? xr_step_bytes(S) : 0.0;
    out4[3] = (double)S.xr.dev_bytes;
}
