// sgrid.inc — sensor bias grids eliminated from the CGNR normal equations (lsq_set_sensor_grids).
// Included by lsqr_cg.inc inside its anonymous namespace, behind bias.inc.
//
// The data rows of grid s gain the unknowns a_s (the grid's node values) with the bilinear weights
// β_i (≤ 4 per row), and the grid is held by the constraint rows C_s a_s = 0.  For fixed x the optimal
// a = M⁻¹ Bᵀ W² (d − A_d x) with M = BᵀW²B + K, K_s = C_sᵀC_s, and substituting it back leaves the
// normal operator N − A_dᵀ W² B M⁻¹ Bᵀ W² A_d.  A row lies in one grid and C_s touches its own nodes
// only: M is one dense SPD block per grid.  On td_i = W_i² (A_d p)_i, which the CG step holds between
// k_cg_dmf_ad and the node gather, the elimination is
//   s = Bᵀ td,   y_s = R_s⁻¹ R_s⁻ᵀ s_s,   td_i −= W_i² Σ_k β_ik y_k,   pᵀNp −= Σ_k s_k y_k
// with M_s = R_sᵀR_s: four launches, whatever the number of grids (k_sg_btd, k_sg_trsv_t, k_sg_trsv,
// k_sg_apply).  M_s is assembled and factored once per solve (the weights and the mask change with
// every outer iteration): k_sg_asm, k_sg_addk, dense_spd_factor per grid.
//
// Reproducibility (SgridData, system.hpp): the transpose by node lists its entries in point order; a
// wave sums them lane-strided and with the fixed shuffle tree; the triangular products add in index
// order.  No atomics: two runs agree bit for bit.
//
// Beside data biases and slopes (lsq_set_sensor_grids_joint) a block also holds the bias IDs and slope
// groups all of whose rows lie in its grid, as dense nodes behind the lattice nodes (SgridData): B gains
// their columns, K their c² on the diagonal, k_sg_asmx forms their entries of M and k_sg_applyx applies
// them; the other IDs and groups stay with bias.inc / slope.inc, and elim_* below runs both.

// the segments of the long dense-node lists (SgridData::seg_*): a wave per segment, lane-strided, then
// the fixed shuffle tree
__global__ __launch_bounds__(BLOCK) void k_sg_btd_seg(const CgState* __restrict__ st, int64_t nseg,
                                                      const int64_t* __restrict__ seg_lo,
                                                      const int64_t* __restrict__ seg_hi,
                                                      const int32_t* __restrict__ tr_pt,
                                                      const double* __restrict__ tr_w, const double* __restrict__ src,
                                                      double* __restrict__ seg_sum) {
    if (st && st->stop) return;
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (BLOCK / 64);
    for (int64_t j = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); j < nseg; j += nw) {   // wave-uniform
        double t = 0.0;
        for (int64_t e = seg_lo[j] + lane; e < seg_hi[j]; e += 64) t += tr_w[e] * src[tr_pt[e]];
        t = wave_sum(t);
        if (lane == 0) seg_sum[j] = t;
    }
}

// s_k = Σ_{e ∈ k} β_e src[pt_e]: a wave per padded node over its transpose entries; seg_ptr (nullable):
// a node with segments adds their sums (k_sg_btd_seg ran before) in segment order instead
__global__ __launch_bounds__(BLOCK) void k_sg_btd(const CgState* __restrict__ st, int64_t ntp,
                                                  const int64_t* __restrict__ tr_ptr,
                                                  const int32_t* __restrict__ tr_pt,
                                                  const double* __restrict__ tr_w, const double* __restrict__ src,
                                                  double* __restrict__ s, const int32_t* __restrict__ seg_ptr,
                                                  const double* __restrict__ seg_sum) {
    if (st && st->stop) return;
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (BLOCK / 64);
    // whole waves leave the loop together: k is wave-uniform
    for (int64_t k = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); k < ntp; k += nw) {
        const int64_t lo = tr_ptr[k], hi = tr_ptr[k + 1];
        const int32_t sa = seg_ptr ? seg_ptr[k] : 0, sb = seg_ptr ? seg_ptr[k + 1] : 0;
        double t = 0.0;
        if (sb > sa)
            for (int32_t j = sa + lane; j < sb; j += 64) t += seg_sum[j];
        else
            for (int64_t e = lo + lane; e < hi; e += 64) t += tr_w[e] * src[tr_pt[e]];
        t = wave_sum(t);
        if (lane == 0) s[k] = t;
    }
}

// z = R⁻ᵀ s per grid: z_j = Σ_{i ≤ j} Ri[i][j] s_i.  A workgroup per 64-column tile of a grid, lane =
// column (coalesced along the rows of Ri); the four waves take the four quarters of the rows
// [0, j0 + 64) (Ri is zero below its diagonal) and their sums are added in wave order.
__global__ __launch_bounds__(BLOCK) void k_sg_trsv_t(const CgState* __restrict__ st, int64_t ntile,
                                                     const int32_t* __restrict__ tile_grid,
                                                     const int32_t* __restrict__ tile_jb,
                                                     const int64_t* __restrict__ poff,
                                                     const int64_t* __restrict__ moff,
                                                     const int64_t* __restrict__ npad, const double* __restrict__ Ri,
                                                     const double* __restrict__ s, double* __restrict__ z) {
    if (st && st->stop) return;
    __shared__ double red[BLOCK];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {   // block-uniform: the barriers see every thread
        const int32_t g = tile_grid[t];
        const int64_t np = npad[g], j0 = (int64_t)tile_jb[t] * 64;
        const double* R = Ri + moff[g];
        const double* sg = s + poff[g];
        const int64_t q = (j0 + 64) / 4;   // a multiple of 16
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int64_t i = w * q; i < (w + 1) * q; i += 4) {
            a0 += R[i * np + j0 + lane] * sg[i];
            a1 += R[(i + 1) * np + j0 + lane] * sg[i + 1];
            a2 += R[(i + 2) * np + j0 + lane] * sg[i + 2];
            a3 += R[(i + 3) * np + j0 + lane] * sg[i + 3];
        }
        red[threadIdx.x] = (a0 + a1) + (a2 + a3);
        __syncthreads();
        if (w == 0) z[poff[g] + j0 + lane] = (red[lane] + red[64 + lane]) + (red[128 + lane] + red[192 + lane]);
        __syncthreads();
    }
}

// y = R⁻¹ z per grid: y_i = Σ_{j ≥ i} Ri[i][j] z_j, a wave per padded node (row), lanes along the row
__global__ __launch_bounds__(BLOCK) void k_sg_trsv(const CgState* __restrict__ st, int64_t ntp,
                                                   const int32_t* __restrict__ node_grid,
                                                   const int64_t* __restrict__ poff,
                                                   const int64_t* __restrict__ moff,
                                                   const int64_t* __restrict__ npad, const double* __restrict__ Ri,
                                                   const double* __restrict__ z, double* __restrict__ y) {
    if (st && st->stop) return;
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (BLOCK / 64);
    for (int64_t k = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); k < ntp; k += nw) {   // wave-uniform
        const int32_t g = node_grid[k];
        const int64_t np = npad[g], i = k - poff[g];
        const double* R = Ri + moff[g] + i * np;
        const double* zg = z + poff[g];
        double t = 0.0;
        for (int64_t j = i / 64 * 64 + lane; j < np; j += 64) t += R[j] * zg[j];   // zeros left of the diagonal
        t = wave_sum(t);
        if (lane == 0) y[k] = t;
    }
}

// mode 0: td_i −= w_i² Σ_k β_ik y_k over the rows that lie in a grid; mode 1: td_i = −(that) (the rows
// outside are zeroed by the caller).  part (nullable): the first npart workgroups also store their
// share of −Σ_k s_k y_k (fixed strides over the padded nodes)
__global__ __launch_bounds__(BLOCK) void k_sg_apply(const CgState* __restrict__ st, int64_t ngp,
                                                    const int32_t* __restrict__ gp_pt,
                                                    const int4* __restrict__ gp_node,
                                                    const double4* __restrict__ gp_wt, const double* __restrict__ w2,
                                                    const double* __restrict__ y, double* __restrict__ td, int mode,
                                                    int64_t ntp, const double* __restrict__ s, double* part,
                                                    int npart) {
    if (st && st->stop) return;
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < ngp; j += (int64_t)gridDim.x * BLOCK) {
        const int32_t i = gp_pt[j];
        const int4 n = gp_node[j];
        const double4 b = gp_wt[j];
        const double d = w2[i] * (((b.x * y[n.x] + b.y * y[n.y]) + b.z * y[n.z]) + b.w * y[n.w]);
        td[i] = mode ? -d : td[i] - d;
    }
    if (part && (int)blockIdx.x < npart) {   // block-uniform
        double acc = 0.0;
        for (int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x; k < ntp; k += (int64_t)npart * BLOCK)
            acc -= s[k] * y[k];
        store_partial(acc, part, blockIdx.x);
    }
}

// k_sg_apply for grids with dense nodes (lsq_set_sensor_grids_joint): a row carries up to three
// further entries, its bias ID's node (coefficient 1) and its slope group's two nodes (u₀, u₁);
// gp_xnode: −1 where the row has none (a row with a group has both of its nodes)
__global__ __launch_bounds__(BLOCK) void k_sg_applyx(const CgState* __restrict__ st, int64_t ngp,
                                                     const int32_t* __restrict__ gp_pt,
                                                     const int4* __restrict__ gp_node,
                                                     const double4* __restrict__ gp_wt,
                                                     const int4* __restrict__ gp_xnode,
                                                     const double2* __restrict__ gp_xu, const double* __restrict__ w2,
                                                     const double* __restrict__ y, double* __restrict__ td, int mode,
                                                     int64_t ntp, const double* __restrict__ s, double* part,
                                                     int npart) {
    if (st && st->stop) return;
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < ngp; j += (int64_t)gridDim.x * BLOCK) {
        const int32_t i = gp_pt[j];
        const int4 n = gp_node[j];
        const double4 b = gp_wt[j];
        const int4 xn = gp_xnode[j];
        const double2 uu = gp_xu[j];
        const double lat = ((b.x * y[n.x] + b.y * y[n.y]) + b.z * y[n.z]) + b.w * y[n.w];
        const double yb = xn.x >= 0 ? y[xn.x] : 0.0;
        const double ys = xn.y >= 0 ? uu.x * y[xn.y] + uu.y * y[xn.z] : 0.0;
        const double d = w2[i] * (lat + (yb + ys));
        td[i] = mode ? -d : td[i] - d;
    }
    if (part && (int)blockIdx.x < npart) {   // block-uniform
        double acc = 0.0;
        for (int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x; k < ntp; k += (int64_t)npart * BLOCK)
            acc -= s[k] * y[k];
        store_partial(acc, part, blockIdx.x);
    }
}

// per solve, dense nodes set: row k of M in its block's dense columns.  A wave per padded node k
// (lattice or dense) walks k's transpose entries; an entry's row adds w² β_k to the column of its ID
// and w² β_k u₀, w² β_k u₁ to the columns of its group: one accumulator per dense slot of the block
// (≤ SG_MAX_DENSE), chosen by compare, then the fixed shuffle tree.  A wave writes its own row only,
// from the diagonal on (dense_spd_factor reads the upper triangle): every entry has one writer and
// one order of summation.  Runs behind k_sg_asm, which left the identity on the dense nodes' rows.
__global__ __launch_bounds__(BLOCK) void k_sg_asmx(int64_t ntp, const int64_t* __restrict__ tr_ptr,
                                                   const int32_t* __restrict__ tr_pt,
                                                   const int32_t* __restrict__ tr_gp,
                                                   const double* __restrict__ tr_w,
                                                   const int4* __restrict__ gp_xnode,
                                                   const double2* __restrict__ gp_xu, const double* __restrict__ w2,
                                                   const int32_t* __restrict__ node_grid,
                                                   const int64_t* __restrict__ poff,
                                                   const int64_t* __restrict__ moff,
                                                   const int64_t* __restrict__ npad, const int64_t* __restrict__ nn,
                                                   const int64_t* __restrict__ nl, const int64_t* __restrict__ nx,
                                                   double* __restrict__ M) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (BLOCK / 64);
    for (int64_t k = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); k < ntp; k += nw) {   // wave-uniform
        const int32_t g = node_grid[k];
        const int64_t np = npad[g], p0 = poff[g], i = k - p0, nlg = nl[g];
        const int nxg = (int)nx[g];
        if (i >= nn[g] || nxg == 0) continue;   // padding, or a block without dense nodes
        const int32_t d0 = (int32_t)(p0 + nlg);   // the block's first dense node
        double acc[SG_MAX_DENSE];
#pragma unroll
        for (int c = 0; c < SG_MAX_DENSE; ++c) acc[c] = 0.0;
        for (int64_t e = tr_ptr[k] + lane; e < tr_ptr[k + 1]; e += 64) {
            const double ww = w2[tr_pt[e]] * tr_w[e];
            const int4 xn = gp_xnode[tr_gp[e]];
            const double2 uu = gp_xu[tr_gp[e]];
            const int s0 = xn.x >= 0 ? xn.x - d0 : -1, s1 = xn.y >= 0 ? xn.y - d0 : -1, s2 = xn.z >= 0 ? xn.z - d0 : -1;
            const double v1 = ww * uu.x, v2 = ww * uu.y;
#pragma unroll
            for (int c = 0; c < SG_MAX_DENSE; ++c) {
                if (s0 == c) acc[c] += ww;
                if (s1 == c) acc[c] += v1;
                if (s2 == c) acc[c] += v2;
            }
        }
        double mine = 0.0;
#pragma unroll
        for (int c = 0; c < SG_MAX_DENSE; ++c) {
            const double t = wave_sum(acc[c]);
            if (lane == c) mine = t;
        }
        if (lane < nxg && nlg + lane >= i) M[moff[g] + i * np + nlg + lane] = mine;
    }
}

// per solve: row k of M = BᵀW²B.  A wave per padded node k walks k's transpose entries; an entry's
// row adds w² β_k β_m to the column of each of its ≤ 4 nodes m, which are among the ≤ SG_NBR nodes
// that share a row with k (tr_slot: their places in nbr).  Padding nodes: the identity.
__global__ __launch_bounds__(BLOCK) void k_sg_asm(int64_t ntp, const int64_t* __restrict__ tr_ptr,
                                                  const int32_t* __restrict__ tr_pt,
                                                  const int32_t* __restrict__ tr_gp,
                                                  const uint32_t* __restrict__ tr_slot,
                                                  const double* __restrict__ tr_w, const double* __restrict__ gp_wt,
                                                  const double* __restrict__ w2, const int32_t* __restrict__ nbr,
                                                  const int32_t* __restrict__ node_grid,
                                                  const int64_t* __restrict__ poff,
                                                  const int64_t* __restrict__ moff,
                                                  const int64_t* __restrict__ npad, const int64_t* __restrict__ nn,
                                                  double* __restrict__ M) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (BLOCK / 64);
    for (int64_t k = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); k < ntp; k += nw) {   // wave-uniform
        const int32_t g = node_grid[k];
        const int64_t np = npad[g], p0 = poff[g], i = k - p0;
        double* row = M + moff[g] + i * np;
        if (i >= nn[g]) {
            if (lane == 0) row[i] = 1.0;
            continue;
        }
        double acc[SG_NBR];
#pragma unroll
        for (int c = 0; c < SG_NBR; ++c) acc[c] = 0.0;
        for (int64_t e = tr_ptr[k] + lane; e < tr_ptr[k + 1]; e += 64) {
            const double ww = w2[tr_pt[e]] * tr_w[e];
            const uint32_t sl = tr_slot[e];
            const double* b = gp_wt + 4 * (int64_t)tr_gp[e];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int slot = (int)((sl >> (8 * q)) & 255u);
                const double v = ww * b[q];
#pragma unroll
                for (int c = 0; c < SG_NBR; ++c)
                    if (slot == c) acc[c] += v;
            }
        }
        double mine = 0.0;
#pragma unroll
        for (int c = 0; c < SG_NBR; ++c) {
            const double t = wave_sum(acc[c]);
            if (lane == c) mine = t;
        }
        if (lane < SG_NBR) {
            const int32_t m = nbr[k * SG_NBR + lane];
            if (m >= 0) row[m - p0] = mine;
        }
    }
}

// per solve: M += K (K's entries are distinct positions: plain read-modify-write)
__global__ __launch_bounds__(BLOCK) void k_sg_addk(int64_t nk, const int64_t* __restrict__ k_pos,
                                                   const double* __restrict__ k_val, double* __restrict__ M) {
    for (int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x; t < nk; t += (int64_t)gridDim.x * BLOCK)
        M[k_pos[t]] += k_val[t];
}

// mode 0 (before the factorisation): d0 = diag M.  mode 1 (after it): err[grid] = 1 where the pivot
// R_kk² is not above SG_PIVOT_REL of M_kk — a grid whose matrix is singular to rounding (the
// factorisation itself flags only pivots ≤ 0, and rounding may leave a tiny positive one)
constexpr double SG_PIVOT_REL = 1e-12;
__global__ __launch_bounds__(BLOCK) void k_sg_diag(int64_t ntp, const int32_t* __restrict__ node_grid,
                                                   const int64_t* __restrict__ poff,
                                                   const int64_t* __restrict__ moff,
                                                   const int64_t* __restrict__ npad, const double* __restrict__ M,
                                                   double* __restrict__ d0, int mode, int* __restrict__ err) {
    for (int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x; k < ntp; k += (int64_t)gridDim.x * BLOCK) {
        const int32_t g = node_grid[k];
        const int64_t i = k - poff[g];
        const double v = M[moff[g] + i * npad[g] + i];
        if (mode == 0)
            d0[k] = v;
        else if (!(v * v > SG_PIVOT_REL * d0[k]))
            err[g] = 1;   // every writer stores the same value
    }
}

// the grids take part in this system's CGNR operator
inline bool sgrid_active(const System& S) { return S.sgrid.on && !S.dist && cg_use_dmf(S); }

// the three launches of y = M⁻¹ Bᵀ src
void sgrid_launch_btd(const System& S, const CgState* st, const double* src) {
    const SgridData& G = S.sgrid;
    if (G.nseg)
        hipLaunchKernelGGL(k_sg_btd_seg, dim3(grid_for(G.nseg, BLOCK / 64)), dim3(BLOCK), 0, S.stream, st, G.nseg,
                           G.seg_lo.p, G.seg_hi.p, G.tr_pt.p, G.tr_w.p, src, G.seg_sum.p);
    hipLaunchKernelGGL(k_sg_btd, dim3(grid_for(G.ntp, BLOCK / 64)), dim3(BLOCK), 0, S.stream, st, G.ntp, G.tr_ptr.p,
                       G.tr_pt.p, G.tr_w.p, src, G.s.p, G.nseg ? G.seg_ptr.p : (const int32_t*)nullptr, G.seg_sum.p);
}

void sgrid_launch_trsv_t(const System& S, const CgState* st) {
    const SgridData& G = S.sgrid;
    hipLaunchKernelGGL(k_sg_trsv_t, dim3(grid_for(G.ntile, 1)), dim3(BLOCK), 0, S.stream, st, G.ntile, G.tile_grid.p,
                       G.tile_jb.p, G.poff.p, G.moff.p, G.npad.p, G.Ri.p, G.s.p, G.z.p);
}

void sgrid_launch_trsv(const System& S, const CgState* st) {
    const SgridData& G = S.sgrid;
    hipLaunchKernelGGL(k_sg_trsv, dim3(grid_for(G.ntp, BLOCK / 64)), dim3(BLOCK), 0, S.stream, st, G.ntp,
                       G.node_grid.p, G.poff.p, G.moff.p, G.npad.p, G.Ri.p, G.z.p, G.y.p);
}

// y = M⁻¹ Bᵀ src (src per sorted point); s and z stay for the partials of k_sg_apply.  marks
// (nullable): the step's stages E0 (s = Bᵀ src), E1 (z = R⁻ᵀ s), E2 (y = R⁻¹ z)
void sgrid_launch_reduce(const System& S, const CgState* st, const double* src, CgMarks* marks = nullptr) {
    sgrid_launch_btd(S, st, src);
    cg_mark(marks, CG_E0, S.stream);
    sgrid_launch_trsv_t(S, st);
    cg_mark(marks, CG_E1, S.stream);
    sgrid_launch_trsv(S, st);
    cg_mark(marks, CG_E2, S.stream);
}

// mode 0: td −= W² B y; mode 1: td = −W² B y (after sgrid_launch_reduce); part (nullable): G.nbk
// partials of −Σ_k s_k y_k
// ngp (≤ G.ngp): 0 stores the partials alone.  Beside the biases (S.bias.on) their apply pass has
// written every row in mode 1 already.
void sgrid_launch_apply(const System& S, const CgState* st, double* td, int mode, double* part, int64_t ngp) {
    const SgridData& G = S.sgrid;
    if (mode && !S.bias.on) HIP_CHECK(hipMemsetAsync(td, 0, sizeof(double) * (size_t)G.npts, S.stream));   // the rows outside every grid
    const int grid = std::max(grid_for(ngp), G.nbk);
    if (G.nxt)
        hipLaunchKernelGGL(k_sg_applyx, dim3(grid), dim3(BLOCK), 0, S.stream, st, ngp, G.gp_pt.p,
                           reinterpret_cast<const int4*>(G.gp_node.p), reinterpret_cast<const double4*>(G.gp_wt.p),
                           reinterpret_cast<const int4*>(G.gp_xnode.p), reinterpret_cast<const double2*>(G.gp_xu.p),
                           G.w2.p, G.y.p, td, mode, G.ntp, G.s.p, part, G.nbk);
    else
        hipLaunchKernelGGL(k_sg_apply, dim3(grid), dim3(BLOCK), 0, S.stream, st, ngp, G.gp_pt.p,
                           reinterpret_cast<const int4*>(G.gp_node.p), reinterpret_cast<const double4*>(G.gp_wt.p), G.w2.p,
                           G.y.p, td, mode, G.ntp, G.s.p, part, G.nbk);
}

// per solve (beside k_dmf_rs): w² per sorted point, M_s = Σ w² β βᵀ + K_s and its factor for the
// current weights / mask.  Throws (naming the grid) when some M_s is not positive definite.
void sgrid_prepare(System& S) {
    SgridData& G = S.sgrid;
    hipStream_t st = S.stream;
    hipLaunchKernelGGL(k_bias_w2, dim3(grid_for(G.npts)), dim3(BLOCK), 0, st, G.npts, S.dmf_perm.p, S.rs.p, G.w2.p);
    G.M.zero(st);
    G.err.zero(st);
    hipLaunchKernelGGL(k_sg_asm, dim3(grid_for(G.ntp, BLOCK / 64)), dim3(BLOCK), 0, st, G.ntp, G.tr_ptr.p, G.tr_pt.p,
                       G.tr_gp.p, G.tr_slot.p, G.tr_w.p, G.gp_wt.p, G.w2.p, G.nbr.p, G.node_grid.p, G.poff.p, G.moff.p,
                       G.npad.p, G.nl.p, G.M.p);   // the lattice nodes; the identity on the dense nodes and the padding
    if (G.nxt)
        hipLaunchKernelGGL(k_sg_asmx, dim3(grid_for(G.ntp, BLOCK / 64)), dim3(BLOCK), 0, st, G.ntp, G.tr_ptr.p,
                           G.tr_pt.p, G.tr_gp.p, G.tr_w.p, reinterpret_cast<const int4*>(G.gp_xnode.p),
                           reinterpret_cast<const double2*>(G.gp_xu.p), G.w2.p, G.node_grid.p, G.poff.p, G.moff.p,
                           G.npad.p, G.nn.p, G.nl.p, G.nx.p, G.M.p);
    if (G.nk) hipLaunchKernelGGL(k_sg_addk, dim3(grid_for(G.nk)), dim3(BLOCK), 0, st, G.nk, G.k_pos.p, G.k_val.p, G.M.p);
    hipLaunchKernelGGL(k_sg_diag, dim3(grid_for(G.ntp)), dim3(BLOCK), 0, st, G.ntp, G.node_grid.p, G.poff.p, G.moff.p,
                       G.npad.p, G.M.p, G.d0.p, 0, G.err.p);
    KERNEL_CHECK();
    for (int64_t g = 0; g < G.ng; ++g)
        dense_spd_factor(G.M.p + G.h_moff[g], G.Ri.p + G.h_moff[g], G.h_npad[g], G.err.p + g, st);
    hipLaunchKernelGGL(k_sg_diag, dim3(grid_for(G.ntp)), dim3(BLOCK), 0, st, G.ntp, G.node_grid.p, G.poff.p, G.moff.p,
                       G.npad.p, G.M.p, G.d0.p, 1, G.err.p);
    KERNEL_CHECK();
    std::vector<int> herr(G.ng, 0);
    G.err.download(herr.data(), G.ng, st);
    HIP_CHECK(hipStreamSynchronize(st));
    for (int64_t g = 0; g < G.ng; ++g)
        if (herr[g])
            throw std::invalid_argument("sensor grid " + std::to_string(g) + ": BᵀW²B + K has a pivot that is not "
                                        "positive (the kept data and the constraints do not determine the grid)");
}

// algorithmic bytes of the step's kernels, out = {s = Bᵀ td, z = R⁻ᵀ s, y = R⁻¹ z, apply}.  Bᵀ td: the
// entries' point, weight and gathered td (20 B), the node pointers and s.  The two triangular products
// each read the upper half of every R_s⁻¹ (with the diagonal tiles whole) and three vectors.  Apply: the
// grid points' index, nodes, weights, w², td read and written (76 B), y gathered within the grid, and
// s, y for the partials.
void sgrid_kernel_bytes(const System& S, double out[4]) {
    const SgridData& G = S.sgrid;
    double tri = 0.0;
    for (int64_t g = 0; g < G.ng; ++g) {
        const double nb = (double)(G.h_npad[g] / 64);
        tri += nb * (nb + 1.0) / 2.0 * 64.0 * 64.0 * 8.0;
    }
    out[0] = 20.0 * (double)G.nent + 16.0 * (double)G.ntp + 32.0 * (double)G.nseg;   // a segment: its bounds, its sum written and read
    out[1] = tri + 16.0 * (double)G.ntp;
    out[2] = tri + 20.0 * (double)G.ntp;
    out[3] = 76.0 * (double)G.ngp + 24.0 * (double)G.ntp;
    if (G.nxt) out[3] += 32.0 * (double)G.ngp;   // the dense entries: three nodes (an int4) and u (nent counts their transpose)
}

double sgrid_step_bytes(const System& S) {
    double k[4];
    sgrid_kernel_bytes(S, k);
    return k[0] + k[1] + k[2] + k[3];
}

// ---- one interface over the two eliminations (biases / slopes, sensor grids, or both) ------------
// Both (lsq_set_sensor_grids_joint): the rows of every grid belong to their block and the others to
// the bias / slope path (its sink rank makes the grids' rows exact zeros there), so the two
// corrections of td touch disjoint rows and add: both reduces read the same td, then both applies
// run.  The partials lie one behind the other: the biases' S.bias.nbk, then the grids' S.sgrid.nbk.
inline int elim_nbk(const System& S) { return (bias_active(S) ? S.bias.nbk : 0) + (sgrid_active(S) ? S.sgrid.nbk : 0); }
inline const double* elim_w2(const System& S) { return S.sgrid.on ? S.sgrid.w2.p : S.bias.w2.p; }
inline int64_t elim_npts(const System& S) { return S.sgrid.on ? S.sgrid.npts : S.bias.npts; }
inline double* elim_sgrid_part(const System& S, double* part) { return part && S.bias.on ? part + S.bias.nbk : part; }

// the eliminated unknowns for the sums of src; part (nullable) as in elim_launch_step.  With sensor
// grids their partials are written by the apply pass: elim_launch_apply must follow with the same part.
// Both set: the marks E0 … E2 stand behind the grids' three launches, E0 spans the bias path's
// reduce as well and E3 (elim_launch_step) both apply passes; with marks->bias_path they stand behind the bias path's three stages, and E3 behind
// its apply pass, so that E3 spans the grids' reduce as well.
void elim_launch_reduce(const System& S, const CgState* st, const double* src, double* part, CgMarks* marks = nullptr) {
    const bool both = S.bias.on && S.sgrid.on, on_bias = marks && marks->bias_path;
    if (S.bias.on) bias_launch_reduce(S, st, src, part, both && !on_bias ? nullptr : marks);
    if (S.sgrid.on) sgrid_launch_reduce(S, st, src, both && on_bias ? nullptr : marks);
}

void elim_launch_apply(const System& S, const CgState* st, double* td, int mode, double* part, CgMarks* marks = nullptr) {
    if (S.bias.on) bias_launch_apply(S, st, td, mode);
    if (S.bias.on && S.sgrid.on && marks && marks->bias_path) cg_mark(marks, CG_E3, S.stream);
    if (S.sgrid.on) sgrid_launch_apply(S, st, td, mode, elim_sgrid_part(S, part), S.sgrid.ngp);
}

// the elimination step on td (W² A_d p per sorted point): td ← W (I − Q) W A_d p; part: elim_nbk
// partials of what the elimination takes off pᵀNp; marks (nullable): the stages E0 … E2 of the reduce
// and E3, the apply pass
void elim_launch_step(const System& S, const CgState* st, double* td, double* part, CgMarks* marks = nullptr) {
    elim_launch_reduce(S, st, td, part, marks);
    elim_launch_apply(S, st, td, 0, part, marks);
    if (!(S.bias.on && S.sgrid.on && marks && marks->bias_path)) cg_mark(marks, CG_E3, S.stream);
}

// the partials alone (the norm of W b in the general start): src is left as it is
void elim_launch_norm(const System& S, const CgState* st, const double* src, double* part) {
    if (S.bias.on) bias_launch_reduce(S, st, src, part);
    if (S.sgrid.on) {
        sgrid_launch_reduce(S, st, src);
        sgrid_launch_apply(S, st, nullptr, 0, elim_sgrid_part(S, part), 0);
    }
}
