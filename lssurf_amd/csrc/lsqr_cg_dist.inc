// lsqr_cg_dist.inc — CGNR (lsq_opts.method = 1) over a Group of structured ranks (y-slab
// windows, lsqr_dist.inc).  Included at the end of lsqr.hip after lsqr_dist.inc.
//
// Every rank holds its window (owned node rows ± halo rows) and the rows anchored in its slab.
// A rank's normal operator N_r = A_rᵀA_r over its window is a structured system like a
// single-GPU one (the column-mode kernels of lsqr_cg.inc run unchanged on it), so per iteration:
//   normal (p over the window from z, β, p_old; q_w = N_s,r p) → data (t = Ad_r p, ‖t‖²) →
//   q_w += ATd_r t → reverse halo of q (ghost partial sums added by their owners, peer order) →
//   all-reduce pᵀAᵀAp = Σ_r (p_wᵀN_s,r p_w + ‖t_r‖²)  [each row lives on one rank] → α →
//   update on owned columns (x, s, z = M⁻¹s; Σ sᵀz) → all-reduce → β → forward halo of z.
// Two halos and two scalar all-reduces per iteration, each all-reduce in the same RCCL group as a
// halo (two communication rounds per iteration; SURVEY.md §8(e)).  Block-Jacobi blocks are
// the window's nodes; their (AᵀA)_bb are summed over the ranks by a reverse halo before the
// owners factor them (group_block_factor), so every N uses the single-GPU preconditioner.
// Jacobi (precond 1) uses the global column norms (group_refresh_mf).

namespace {

// block b's packed (AᵀA)_bb partial (upper, e = j(j+1)/2 + i) -> per-column arrays:
// tmp[k·nf + col_j] = N_b(k, j) for every row k of the block
__global__ __launch_bounds__(BLOCK) void k_blk_to_cols(int64_t nb, int npk, const int64_t* __restrict__ ptr,
                                                       const int32_t* __restrict__ full, const double* __restrict__ Ri,
                                                       int64_t nf, double* __restrict__ tmp) {
    for (int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x; q < nb * BJ_LANES; q += (int64_t)gridDim.x * BLOCK) {
        const int64_t b = q / BJ_LANES;
        const int j = (int)(q - b * BJ_LANES);
        const int kb = (int)(ptr[b + 1] - ptr[b]);
        if (j >= kb) continue;
        const int32_t c = full[ptr[b] + j];
        const double* R = Ri + b * npk;
        for (int k = 0; k < kb; ++k) tmp[(int64_t)k * nf + c] = k <= j ? R[j * (j + 1) / 2 + k] : R[k * (k + 1) / 2 + j];
    }
}

// the reverse: packed N_b(i, j) = tmp[i·nf + col_j]
__global__ __launch_bounds__(BLOCK) void k_cols_to_blk(int64_t nb, int npk, const int64_t* __restrict__ ptr,
                                                       const int32_t* __restrict__ full, const double* __restrict__ tmp,
                                                       int64_t nf, double* __restrict__ Ri) {
    for (int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x; q < nb * npk; q += (int64_t)gridDim.x * BLOCK) {
        const int64_t b = q / npk;
        const int e = (int)(q - b * npk);
        int j = 0;
        while ((j + 1) * (j + 2) / 2 <= e) ++j;
        const int i = e - j * (j + 1) / 2;
        const int kb = (int)(ptr[b + 1] - ptr[b]);
        Ri[q] = j < kb ? tmp[(int64_t)i * nf + full[ptr[b] + j]] : 0.0;
    }
}

double* sel_blktmp(System& S, int k) { return S.blk_tmp.p + (int64_t)k * S.n_full; }

// Block-Jacobi factors of the owned node blocks from the FULL (AᵀA)_bb: each rank forms the
// partial blocks of every window block from its own rows, ghost blocks' partials are added into
// their owners' blocks by the reverse halo (one pass per block row), then the owners factor.
// The blocks of a node list its columns in the same (global) order on every rank.
void group_block_factor(Group& G) {
    int kmax = 1;
    for (System* S : G.ranks) {
        ensure_blocks(*S);
        kmax = std::max(kmax, S->blk_kmax);
    }
    for (System* S : G.ranks) {
        const int npk = S->blk_kmax * (S->blk_kmax + 1) / 2;
        if (S->blk_Ri.n != (int64_t)npk * S->nblk) S->blk_Ri.alloc((int64_t)npk * S->nblk);
        block_normal(*S);
        const int64_t nf = S->n_full;
        if (S->blk_tmp.n != (int64_t)kmax * nf) S->blk_tmp.alloc((int64_t)kmax * nf);
        S->blk_tmp.zero(S->stream);
        hipLaunchKernelGGL(k_blk_to_cols, dim3(grid_for(S->nblk * BJ_LANES)), dim3(BLOCK), 0, S->stream, S->nblk, npk,
                           S->blk_ptr.p, S->blk_full.p, S->blk_Ri.p, nf, S->blk_tmp.p);
        KERNEL_CHECK();
    }
    for (int k = 0; k < kmax; ++k) group_halo_rev_idx(G, sel_blktmp, k);
    for (System* S : G.ranks) {
        const int npk = S->blk_kmax * (S->blk_kmax + 1) / 2;
        hipLaunchKernelGGL(k_cols_to_blk, dim3(grid_for(S->nblk * npk)), dim3(BLOCK), 0, S->stream, S->nblk, npk,
                           S->blk_ptr.p, S->blk_full.p, S->blk_tmp.p, S->n_full, S->blk_Ri.p);
        KERNEL_CHECK();
        block_factor_in_place(*S);
        S->blk_tmp = DBuf<double>();
    }
}

double* sel_cgq(System& S, int) { return S.cg_q.p; }
double* sel_cgs(System& S, int) { return S.cg_s.p; }
double* sel_cgz(System& S, int) { return S.cg_z.p; }

// ---- multigrid over ranks (precond 4) ---------------------------------------------------------
// Level 0 of the V-cycle is each rank's window (the single-GPU level-0 kernels on it; the operator
// is the rank's partial N, completed by a forward halo of its operand and a reverse halo of q, as
// in the CG step; the smoothing passes update owned columns only).  The restriction of the owned
// rows into the GLOBAL level 1 is summed over the ranks (one vector all-reduce per cycle); levels
// ≥ 1 are the global Galerkin levels, replicated on every rank (identical tables, lumped data rows
// summed once per solve), so every rank runs the same coarse cycle and prolongs into its window.
// In exact arithmetic this is the single-GPU V-cycle: same preconditioner, same iteration count.

__global__ __launch_bounds__(BLOCK) void k_group_vec_reduce(double* const* __restrict__ v, int nranks, int64_t n,
                                                            int max) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        double s = v[0][i];
        for (int r = 1; r < nranks; ++r) s = max ? fmax(s, v[r][i]) : s + v[r][i];   // rank order
        for (int r = 0; r < nranks; ++r) v[r][i] = s;
    }
}

using RankVec = double* (*)(System&);
// v ← Σ_ranks v (max: elementwise max), in place on every rank
void group_allreduce_vec(Group& G, RankVec sel, int64_t n, bool max = false) {
    if (n <= 0) return;
    if (G.virt) {
        std::vector<double*> ptrs;
        for (System* S : G.ranks) ptrs.push_back(sel(*S));
        System& S0 = *G.ranks[0];
        if (G.vec_ptrs.n != (int64_t)ptrs.size()) G.vec_ptrs.alloc((int64_t)ptrs.size());
        G.vec_ptrs.upload(ptrs.data(), (int64_t)ptrs.size(), S0.stream);
        hipLaunchKernelGGL(k_group_vec_reduce, dim3(grid_for(n)), dim3(BLOCK), 0, S0.stream, G.vec_ptrs.p,
                           (int)ptrs.size(), n, max ? 1 : 0);
        KERNEL_CHECK();
        HIP_CHECK(hipStreamSynchronize(S0.stream));   // vec_ptrs is reused by the next call
        return;
    }
    group_fence(G);
    NCCL_CHECK(ncclGroupStart());
    for (System* S : G.ranks)
        NCCL_CHECK(ncclAllReduce(sel(*S), sel(*S), (size_t)n, ncclFloat64, max ? ncclMax : ncclSum, S->comm, S->stream));
    NCCL_CHECK(ncclGroupEnd());
}

double* sel_dgw(System& S) { return S.dg_w.p; }
double* sel_lump1(System& S) { return S.mg->lev[1].B.p; }
double* sel_vz1(System& S) { return S.mg->lev[1].vz.p; }
double* sel_r1(System& S) { return S.mg->lev[1].r.p; }
double* sel_d0(System& S, int) { return S.mg->d0.p; }

// ---- partitioned coarse levels --------------------------------------------------------------
// Levels 1 … lp are split over the ranks like level 0: a rank owns the coarse node rows its fine
// rows' even nodes sit on (oa_ℓ = ⌈oa_{ℓ−1} / 2⌉, the last rank up to the level's end), computes
// the operator, smoothing and restriction for those rows only, and exchanges boundary rows with
// its two neighbours: a forward halo of the level's x (the stencil reach, 2 rows) before every
// operator application, a reverse halo of the restricted right-hand side (its partial sums for
// the neighbours' rows, 1 row) and a forward halo of the coarse x before the prolongation (1 row).
// The vectors stay global (each rank holds the whole level; only its rows ± the halo are current),
// so the kernels keep the global geometry and class tables and take a row range.  Levels below lp
// (fewer than LSQ_MG_PART_MIN rows on some rank) are replicated as before: the restriction into the
// first of them is summed over the ranks by one all-reduce of that (small) level.
// In exact arithmetic this is the single-GPU V-cycle.

constexpr int MG_PART_MIN = 8;   // node rows a rank must own on a partitioned level (LSQ_MG_PART_MIN)

__host__ __device__ inline int64_t mg_rows_count(const MgGeom& G, int d) { return (int64_t)d * G.S1 * ((G.has_z ? 1 : 0) + G.nt); }

// rows [y0, y0 + d) of a level vector ↔ a packed buffer (the z0 block's rows, then the dz block's)
__global__ __launch_bounds__(BLOCK) void k_mg_rows_pack(MgGeom G, int y0, int d, const double* __restrict__ v,
                                                        double* __restrict__ buf) {
    const int64_t nz = G.has_z ? (int64_t)d * G.S1 : 0, n = mg_rows_count(G, d);
    for (int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x; k < n; k += (int64_t)gridDim.x * BLOCK)
        buf[k] = k < nz ? v[G.colz + (int64_t)y0 * G.S1 + k] : v[G.cold + (int64_t)y0 * G.S1 * G.nt + (k - nz)];
}
__global__ __launch_bounds__(BLOCK) void k_mg_rows_unpack(MgGeom G, int y0, int d, const double* __restrict__ buf,
                                                          double* __restrict__ v, int add) {
    const int64_t nz = G.has_z ? (int64_t)d * G.S1 : 0, n = mg_rows_count(G, d);
    for (int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x; k < n; k += (int64_t)gridDim.x * BLOCK) {
        const int64_t c = k < nz ? G.colz + (int64_t)y0 * G.S1 + k : G.cold + (int64_t)y0 * G.S1 * G.nt + (k - nz);
        v[c] = add ? v[c] + buf[k] : buf[k];
    }
}

double* sel_pcnt(System& S) { return S.mg->part_t.p; }

// which coarse levels are split: every rank must own ≥ LSQ_MG_PART_MIN rows (and ≥ the halo depth),
// the level must run the tile / direct operator kernels (row ranges) and not be the coarsest
void group_mg_partition(Group& G) {
    static const int pmin = getenv("LSQ_MG_PART_MIN") ? std::max(2, atoi(getenv("LSQ_MG_PART_MIN"))) : MG_PART_MIN;
    static const bool on = !(getenv("LSQ_MG_PART") && getenv("LSQ_MG_PART")[0] == '0');
    const int L = (int)G.ranks[0]->mg->lev.size();
    for (System* S : G.ranks) {
        MgHier& H = *S->mg;
        H.lp = 0;
        std::vector<double> negcnt(L, 0.0);
        int oa = H.oa, ob = H.ob, S0p = H.g0g.S0;
        for (int l = 1; l < L; ++l) {
            MgLevel& V = H.lev[l];
            oa = oa == 0 ? 0 : (oa + 1) / 2;
            ob = ob == S0p ? V.geo.S0 : (ob + 1) / 2;
            S0p = V.geo.S0;
            V.oa = oa;
            V.ob = ob;
            negcnt[l] = -(double)(ob - oa);
        }
        if (H.part_t.n < L) H.part_t.alloc(std::max<int64_t>(L, NPART));
        H.part_t.upload(negcnt.data(), L, S->stream);
        HIP_CHECK(hipStreamSynchronize(S->stream));
    }
    group_allreduce_vec(G, sel_pcnt, L, true);   // max of −count = −(the fewest rows any rank owns)
    for (System* S : G.ranks) {
        MgHier& H = *S->mg;
        std::vector<double> negmin(L);
        H.part_t.download(negmin.data(), L, S->stream);
        HIP_CHECK(hipStreamSynchronize(S->stream));
        int lp = 0;
        const int nr = G.virt ? (int)G.ranks.size() : S->nranks;
        for (int l = 1; on && nr > 1 && l < L; ++l) {
            const MgLevel& V = H.lev[l];
            const int d = std::max(V.tz.hy, V.td.hy);
            if (V.coarsest || !(V.tile || V.direct) || -negmin[l] < std::max(pmin, d)) break;
            lp = l;
        }
        H.lp = lp;
        for (int l = 1; l <= lp; ++l) {
            MgLevel& V = H.lev[l];
            const int64_t cnt = mg_rows_count(V.geo, 2);
            if (V.hb.n != 4 * cnt) V.hb.alloc(4 * cnt);
        }
    }
}

// a partitioned level's row halo: fwd — the owned boundary rows (d of them) into the neighbours'
// copies of those rows; rev — the rank's partial sums in the row beside its owned ones (d = 1) added
// into the neighbour's owned row.  vec(S) selects the level vector of each rank.
template <class Vec>
void group_mg_rows_halo(Group& G, int l, Vec vec, int d, bool rev) {
    for (System* S : G.ranks) {
        MgLevel& V = S->mg->lev[l];
        const int64_t cnt = mg_rows_count(V.geo, d), stride = V.hb.n / 4;
        double* b = V.hb.p;   // [send lower | send upper | recv lower | recv upper]
        const int g = grid_for(cnt);
        if (V.oa > 0)
            hipLaunchKernelGGL(k_mg_rows_pack, dim3(g), dim3(BLOCK), 0, S->stream, V.geo, rev ? V.oa - d : V.oa, d, vec(*S),
                               b);
        if (V.ob < V.geo.S0)
            hipLaunchKernelGGL(k_mg_rows_pack, dim3(g), dim3(BLOCK), 0, S->stream, V.geo, rev ? V.ob : V.ob - d, d, vec(*S),
                               b + stride);
        KERNEL_CHECK();
    }
    if (G.virt) {
        for (size_t r = 0; r < G.ranks.size(); ++r) {
            System& S = *G.ranks[r];
            MgLevel& V = S.mg->lev[l];
            const int64_t cnt = mg_rows_count(V.geo, d), stride = V.hb.n / 4;
            if (V.oa > 0) {   // → the lower neighbour's "recv upper"
                MgLevel& W = G.ranks[r - 1]->mg->lev[l];
                HIP_CHECK(hipMemcpyAsync(W.hb.p + 3 * (W.hb.n / 4), V.hb.p, sizeof(double) * cnt, hipMemcpyDeviceToDevice,
                                         S.stream));
            }
            if (V.ob < V.geo.S0) {   // → the upper neighbour's "recv lower"
                MgLevel& W = G.ranks[r + 1]->mg->lev[l];
                HIP_CHECK(hipMemcpyAsync(W.hb.p + 2 * (W.hb.n / 4), V.hb.p + stride, sizeof(double) * cnt,
                                         hipMemcpyDeviceToDevice, S.stream));
            }
        }
    } else {
        group_fence(G);
        NCCL_CHECK(ncclGroupStart());
        for (System* S : G.ranks) {
            MgLevel& V = S->mg->lev[l];
            const int64_t cnt = mg_rows_count(V.geo, d), stride = V.hb.n / 4;
            if (V.oa > 0) {
                NCCL_CHECK(ncclSend(V.hb.p, (size_t)cnt, ncclFloat64, S->rank - 1, S->comm, S->stream));
                NCCL_CHECK(ncclRecv(V.hb.p + 2 * stride, (size_t)cnt, ncclFloat64, S->rank - 1, S->comm, S->stream));
            }
            if (V.ob < V.geo.S0) {
                NCCL_CHECK(ncclSend(V.hb.p + stride, (size_t)cnt, ncclFloat64, S->rank + 1, S->comm, S->stream));
                NCCL_CHECK(ncclRecv(V.hb.p + 3 * stride, (size_t)cnt, ncclFloat64, S->rank + 1, S->comm, S->stream));
            }
        }
        NCCL_CHECK(ncclGroupEnd());
    }
    for (System* S : G.ranks) {
        MgLevel& V = S->mg->lev[l];
        const int64_t cnt = mg_rows_count(V.geo, d), stride = V.hb.n / 4;
        const int g = grid_for(cnt);
        if (V.oa > 0)
            hipLaunchKernelGGL(k_mg_rows_unpack, dim3(g), dim3(BLOCK), 0, S->stream, V.geo, rev ? V.oa : V.oa - d, d,
                               V.hb.p + 2 * stride, vec(*S), rev ? 1 : 0);
        if (V.ob < V.geo.S0)
            hipLaunchKernelGGL(k_mg_rows_unpack, dim3(g), dim3(BLOCK), 0, S->stream, V.geo, rev ? V.ob - d : V.ob, d,
                               V.hb.p + 3 * stride, vec(*S), rev ? 1 : 0);
        KERNEL_CHECK();
    }
}

int mg_halo_depth(const MgLevel& V) { return std::max(1, std::max(V.tz.hy, V.td.hy)); }

double* sel_rfirst(System& S) { return S.mg->lev[S.mg->lp + 1].r.p; }

// the V-cycle on a partitioned level l (1 ≤ l ≤ lp), its right-hand side complete on the owned rows
void group_mg_cycle_part(Group& G, int l) {
    MgHier& H0 = *G.ranks[0]->mg;
    const int deg = H0.deg, lp = H0.lp;
    const int d = mg_halo_depth(H0.lev[l]);
    auto vx = [l](System& S) { return S.mg->lev[l].x.p; };
    auto op = [&](int) {
        group_mg_rows_halo(G, l, vx, d, false);
        for (System* S : G.ranks) {
            MgHier& H = *S->mg;
            MgLevel& V = H.lev[l];
            mg_launch_op(*S, H, l, S->cst.p, V.x.p, nullptr, H.scal.p + 1, nullptr, V.q.p, V.oa, V.ob);
        }
    };
    auto smooth = [&](int mode, int step) {
        for (System* S : G.ranks) {
            MgHier& H = *S->mg;
            MgLevel& V = H.lev[l];
            mg_launch_smooth(*S, H, l, S->cst.p, mg_vecs(*S, H, l), mode, step, nullptr, nullptr,
                             (int64_t)V.oa * V.geo.S1, (int64_t)V.ob * V.geo.S1);
        }
    };
    smooth(MG_XZERO | (deg <= 2 ? MG_NOD : 0), 0);
    for (int k = 1; k < deg; ++k) {
        op(k);
        smooth((k == 1 ? MG_DX : 0) | (k == deg - 1 ? MG_NOD : 0), k);
    }
    op(0);
    smooth(MG_RES, 0);   // res = r − q − B x on the owned rows
    const int lc = l + 1;
    for (System* S : G.ranks) {
        MgHier& H = *S->mg;
        MgLevel &V = H.lev[l], &C = H.lev[lc];
        // partitioned coarse level: the rows the owned fine rows reach; replicated: all of it (the
        // other ranks' rows 0), summed below
        const int ca = lc <= lp ? std::max(0, C.oa - 1) : 0, cb = lc <= lp ? std::min(C.geo.S0, C.ob + 1) : C.geo.S0;
        const int64_t nr = mg_rows_count(C.geo, cb - ca);
        hipLaunchKernelGGL(k_mg_restrict_win, dim3(grid_for(nr)), dim3(BLOCK), 0, S->stream, S->cst.p, V.geo, C.geo, 0,
                           V.oa, V.ob, V.res.p, nullptr, C.r.p, ca, cb);
        KERNEL_CHECK();
    }
    if (lc <= lp) {
        group_mg_rows_halo(G, lc, [lc](System& S) { return S.mg->lev[lc].r.p; }, 1, true);
        group_mg_cycle_part(G, lc);
        group_mg_rows_halo(G, lc, [lc](System& S) { return S.mg->lev[lc].x.p; }, 1, false);
    } else {
        group_allreduce_vec(G, sel_rfirst, H0.lev[lc].geo.n_full);
        for (System* S : G.ranks) mg_vcycle_graph(*S, *S->mg, lc);
    }
    for (System* S : G.ranks) {
        MgHier& H = *S->mg;
        MgLevel &V = H.lev[l], &C = H.lev[lc];
        hipLaunchKernelGGL(k_mg_prolong_win, dim3(grid_for(V.geo.n_full)), dim3(BLOCK), 0, S->stream, S->cst.p, V.geo,
                           C.geo, 0, C.x.p, V.x.p, V.oa, V.ob);
        KERNEL_CHECK();
    }
    for (int k = 0; k < deg; ++k) {
        op(k);
        smooth((k == deg - 1 ? MG_NOD : 0), k);
    }
}

// λ of the partitioned levels: the single-GPU power steps with each rank's rows, the level's halo
// before every operator application and the Rayleigh sums all-reduced (gsum slots 8, 9)
void group_mg_power_part(Group& G) {
    const int lp = G.ranks[0]->mg->lp;
    for (int l = 1; l <= lp; ++l) {
        const int d = mg_halo_depth(G.ranks[0]->mg->lev[l]);
        for (System* S : G.ranks) {
            MgHier& H = *S->mg;
            MgLevel& V = H.lev[l];
            hipLaunchKernelGGL(k_mg_randvec, dim3(grid_for(V.geo.n_full)), dim3(BLOCK), 0, S->stream, V.geo, V.geo,
                               (int64_t)0, V.d.p);
            HIP_CHECK(hipMemsetAsync(H.scal.p, 0, 2 * sizeof(double), S->stream));
            KERNEL_CHECK();
        }
        for (int k = 0; k < MG_POW; ++k) {
            group_mg_rows_halo(G, l, [l](System& S) { return S.mg->lev[l].d.p; }, d, false);
            for (System* S : G.ranks) {
                MgHier& H = *S->mg;
                MgLevel& V = H.lev[l];
                const int64_t n0 = (int64_t)V.oa * V.geo.S1, n1 = (int64_t)V.ob * V.geo.S1;
                mg_launch_op(*S, H, l, H.mst.p, V.d.p, V.d.p, H.scal.p, V.x.p, V.q.p, V.oa, V.ob);
                const MgVec vp = {V.r.p, V.x.p, V.q.p, V.d.p, V.res.p};
                mg_launch_smooth(*S, H, l, H.mst.p, vp, MG_POWER, 0, H.part1.p, H.part2.p, n0, n1);
                const int gb = mg_grid_blocks(n1 - n0);
                hipLaunchKernelGGL(k_red_parts, dim3(1), dim3(BLOCK), 0, S->stream, H.part1.p, gb, 8, H.part2.p, gb, 9,
                                   S->gsum.p);
            }
            group_allreduce(G, 8, 2);
            for (System* S : G.ranks) {
                MgHier& H = *S->mg;
                hipLaunchKernelGGL(k_mg_power_scalar, dim3(1), dim3(BLOCK), 0, S->stream, S->gsum.p + 8, S->gsum.p + 9, 1,
                                   k, H.lam.p + l, H.scal.p);
            }
        }
        for (System* S : G.ranks) {
            MgHier& H = *S->mg;
            H.lev[l].x.zero(S->stream);
            H.lev[l].d.zero(S->stream);
            HIP_CHECK(hipMemsetAsync(H.scal.p, 0, 2 * sizeof(double), S->stream));
        }
    }
}

// the ranks' hierarchies: the global parts' row scales (a rank without rows of a part contributes
// 0; max over ranks), global level-0 tables, each rank's window level 0 + replicated coarse levels,
// the field-valued rows of level 1 summed
void group_mg_build(Group& G) {
    for (System* S : G.ranks)
        if (!S->dg_on) throw std::invalid_argument("multigrid over ranks needs lsq_dist_set_global on every rank");
    const int np = G.ranks[0]->dg_mfh.n_parts;
    for (System* S : G.ranks) {
        if (S->dg_mfh.n_parts != np || (int)S->dg_local.size() != np)
            throw std::invalid_argument("multigrid over ranks: the ranks' global descriptions differ");
        std::vector<double> w(std::max(np, 1), 0.0);
        for (int p = 0; p < np; ++p) {
            const int l = S->dg_local[p];
            if (l >= 0) {
                if (!S->mfh.p[l].wconst) throw std::invalid_argument("multigrid over ranks: per-row constraint scales");
                w[p] = S->mfh.p[l].w;
            }
        }
        if (S->dg_w.n != (int64_t)w.size()) S->dg_w.alloc((int64_t)w.size());
        S->dg_w.upload(w.data(), (int64_t)w.size(), S->stream);
        HIP_CHECK(hipStreamSynchronize(S->stream));
    }
    group_allreduce_vec(G, sel_dgw, np, true);
    for (System* S : G.ranks) {
        std::vector<double> w(std::max(np, 1));
        S->dg_w.download(w.data(), (int64_t)w.size(), S->stream);
        HIP_CHECK(hipStreamSynchronize(S->stream));
        MfDesc d = S->dg_mfh;
        for (int p = 0; p < np; ++p) {
            d.p[p].w = w[p];
            d.p[p].wconst = 1;
        }
        MgDistInfo di;
        di.T0.resize(d.n_grids);
        std::string why;
        for (int g = 0; g < d.n_grids; ++g)
            if (!ns_from_parts(d, g, di.T0[g], why)) throw std::invalid_argument("multigrid over ranks: " + why);
        di.S0g = S->dg_S0;
        di.wa = S->dg_wa;
        di.oa = S->dg_oa;
        di.ob = S->dg_ob;
        mg_free(S->mg);
        S->mg = nullptr;
        S->mg_why.clear();
        if (!mg_build(*S, S->mg_why, &di)) throw std::invalid_argument("multigrid over ranks: " + S->mg_why);
    }
    const size_t L = G.ranks[0]->mg->lev.size();
    for (System* S : G.ranks)
        if (S->mg->lev.size() != L) throw std::logic_error("multigrid over ranks: the ranks' hierarchies differ");
    if (G.ranks[0]->mg->var) {
        group_allreduce_vec(G, sel_vz1, G.ranks[0]->mg->lev[1].geo.nodes * MG_VN);
        for (System* S : G.ranks) mg_var_coarse(*S);
    }
    group_mg_partition(G);
}

// level-0 operator of the ranks: q = N x over the owned columns (x on the window: the forward halo
// first when the ghosts are stale)
void group_mg_op0(Group& G, bool fwd) {
    if (fwd) group_halo_fwd_idx(G, sel_cgz, 0);
    for (System* S : G.ranks) {
        MgHier& H = *S->mg;
        mg_launch_op(*S, H, 0, S->cst.p, S->cg_z.p, nullptr, H.scal.p + 1, nullptr, S->cg_q.p);
    }
    group_halo_rev_idx(G, sel_cgq, 0);
}

// per-solve set-up over ranks: level-1 lumped data summed, the local coarse set-up, λ of level 0 by
// power steps with halos and all-reduced sums (gsum slots 8, 9)
void group_mg_setup(Group& G) {
    for (System* S : G.ranks) {
        S->mg->lev[1].B.zero(S->stream);
        mg_setup_lump1(*S);
    }
    group_allreduce_vec(G, sel_lump1, G.ranks[0]->mg->lev[1].geo.nodes * G.ranks[0]->mg->nbB);
    for (System* S : G.ranks) mg_setup_rest(*S, S->mg->lp + 1);   // λ of the replicated levels
    group_mg_power_part(G);                                        // λ of the partitioned ones
    for (System* S : G.ranks) {
        MgHier& H = *S->mg;
        const MgLevel& V = H.lev[0];
        hipLaunchKernelGGL(k_mg_randvec, dim3(grid_for(V.geo.n_full)), dim3(BLOCK), 0, S->stream, V.geo, H.g0g,
                           (int64_t)H.wa * V.geo.S1, H.d0.p);
        HIP_CHECK(hipMemsetAsync(H.scal.p, 0, 2 * sizeof(double), S->stream));
        KERNEL_CHECK();
    }
    for (int k = 0; k < MG_POW; ++k) {
        group_halo_fwd_idx(G, sel_d0, 0);
        for (System* S : G.ranks) {
            MgHier& H = *S->mg;
            mg_launch_op(*S, H, 0, H.mst.p, H.d0.p, H.d0.p, H.scal.p, H.res0.p, S->cg_q.p);
        }
        group_halo_rev_idx(G, sel_cgq, 0);
        for (System* S : G.ranks) {
            MgHier& H = *S->mg;
            const MgVec v0 = mg_vecs(*S, H, 0);
            const MgVec vp = {v0.r, H.res0.p, S->cg_q.p, H.d0.p, v0.res};
            mg_launch_smooth(*S, H, 0, H.mst.p, vp, MG_POWER, 0, H.part1.p, H.part2.p);
            hipLaunchKernelGGL(k_red_parts, dim3(1), dim3(BLOCK), 0, S->stream, H.part1.p, H.lev[0].gB, 8, H.part2.p,
                               H.lev[0].gB, 9, S->gsum.p);
        }
        group_allreduce(G, 8, 2);
        for (System* S : G.ranks) {
            MgHier& H = *S->mg;
            hipLaunchKernelGGL(k_mg_power_scalar, dim3(1), dim3(BLOCK), 0, S->stream, S->gsum.p + 8, S->gsum.p + 9, 1, k,
                               H.lam.p, H.scal.p);
        }
    }
    for (System* S : G.ranks) {
        MgHier& H = *S->mg;
        HIP_CHECK(hipMemsetAsync(H.scal.p, 0, 2 * sizeof(double), S->stream));
        H.res0.zero(S->stream);
        H.d0.zero(S->stream);
        S->cg_q.zero(S->stream);
        HIP_CHECK(hipStreamSynchronize(S->stream));
    }
}

// the V-cycle preconditioner of a CG step over ranks: s −= αq, x every CG_XK-th step and
// z = c₂M⁻¹s (k_cg_block, owned columns), then level 0 with halos,
// the summed restriction, the replicated coarse cycle, the prolongation, post-smoothing; the last
// smoothing pass leaves the ρ partials in cg_part_r (the caller all-reduces them with the z halo)
void group_mg_precond(Group& G) {
    for (size_t r = 0; r < G.ranks.size(); ++r) {
        System& S = *G.ranks[r];
        cg_launch_block(S, cg_grids(S, 3), cg_pbufs(S), S.cg_z.p, S.mg->lam.p);
    }
    const int deg = G.ranks[0]->mg->deg0;
    for (int k = 1; k < deg; ++k) {
        group_mg_op0(G, true);
        for (System* S : G.ranks) {
            MgHier& H = *S->mg;
            mg_launch_smooth(*S, H, 0, S->cst.p, mg_vecs(*S, H, 0), (k == 1 ? MG_DX : 0) | (k == deg - 1 ? MG_NOD : 0), k,
                             nullptr, nullptr);
        }
    }
    group_mg_op0(G, true);
    const int lp = G.ranks[0]->mg->lp;
    for (System* S : G.ranks) {
        MgHier& H = *S->mg;
        const MgGeom &F = H.lev[0].geo, &C = H.lev[1].geo;
        // level 1 partitioned: the coarse rows the owned fine rows reach (ghost partials to their
        // owners by the reverse halo); replicated: the whole level, summed over the ranks
        const MgLevel& V1 = H.lev[1];
        const int ca = lp ? std::max(0, V1.oa - 1) : 0, cb = lp ? std::min(C.S0, V1.ob + 1) : C.S0;
        const int64_t nr = mg_rows_count(C, cb - ca);
        hipLaunchKernelGGL(k_mg_restrict_win, dim3(grid_for(nr)), dim3(BLOCK), 0, S->stream, S->cst.p, F, C, H.wa,
                           H.oa, H.ob, S->cg_s.p, S->cg_q.p, H.lev[1].r.p, ca, cb);
    }
    if (lp) {
        group_mg_rows_halo(G, 1, [](System& S) { return S.mg->lev[1].r.p; }, 1, true);
        group_mg_cycle_part(G, 1);
        group_mg_rows_halo(G, 1, [](System& S) { return S.mg->lev[1].x.p; }, 1, false);
    } else {
        group_allreduce_vec(G, sel_r1, G.ranks[0]->mg->lev[1].geo.n_full);
        for (System* S : G.ranks) mg_vcycle_graph(*S, *S->mg, 1);
    }
    for (System* S : G.ranks) {
        MgHier& H = *S->mg;
        // replicated level 1: every window row (the ghosts then hold their owners' values);
        // partitioned: the owned rows (the ghosts come with the next operator's halo)
        const int fa = lp ? H.oa : H.wa, fb = lp ? H.ob : H.wa + H.lev[0].geo.S0;
        hipLaunchKernelGGL(k_mg_prolong_win, dim3(grid_for(H.lev[0].geo.n_full)), dim3(BLOCK), 0, S->stream, S->cst.p,
                           H.lev[0].geo, H.lev[1].geo, H.wa, H.lev[1].x.p, S->cg_z.p, fa, fb);
    }
    for (int k = 0; k < deg; ++k) {
        group_mg_op0(G, k > 0 || lp > 0);   // replicated level 1: after the prolongation the ghosts hold their owners' values
        for (System* S : G.ranks) {
            MgHier& H = *S->mg;
            const bool last = k == deg - 1;
            mg_launch_smooth(*S, H, 0, S->cst.p, mg_vecs(*S, H, 0), (last ? MG_RHO : 0) | (last ? MG_NOD : 0), k,
                             last ? S->cg_part_r.p : nullptr, nullptr);
        }
    }
}

void group_cg_prepare(Group& G, int precond) {
    if (precond != 1 && precond != 3 && precond != 4)
        throw std::invalid_argument("CGNR: precond must be 1 (Jacobi), 3 (block-Jacobi) or 4 (multigrid)");
    for (System* S : G.ranks)
        if (!S->dist_mf) throw std::invalid_argument("CGNR over ranks needs structured ranks (lsq_dist_set_halo)");
    const int pr = precond == 4 ? 3 : precond;   // the V-cycle smooths with the block-Jacobi factors
    group_refresh_mf(G, pr);   // row scales, part scales; csf: global column norms (1) or the live mask (3)
    bool stale = false;
    for (System* S : G.ranks) stale |= pr == 3 && !S->blk_valid;
    if (stale) group_block_factor(G);
    bool build = false;
    for (System* S : G.ranks) {
        if (!cg_prepare(*S, precond)) throw std::invalid_argument("CGNR not available on a rank: " + S->cg_why);
        if (!S->cgh.colmode) throw std::invalid_argument("CGNR over ranks needs the column-mode normal operator");
        build |= precond == 4 && !S->mg;
    }
    if (build) group_mg_build(G);
}

CgState group_cg_state(Group& G) {
    CgState h{};
    System& S = *G.ranks[0];
    HIP_CHECK(hipMemcpyAsync(&h, S.cst.p, sizeof(h), hipMemcpyDeviceToHost, S.stream));
    for (System* R : G.ranks) HIP_CHECK(hipStreamSynchronize(R->stream));
    return h;   // identical on every rank: the scalars come from all-reduced sums
}

// s0 = Aᵀ(W b − A x0) assembled on the owners, z0 = M⁻¹ s0, ρ0; z0 mirrored to the ghosts.
// h_x0 (nullable): per rank, x0 on every local compact column (owned and ghost: the ghosts hold
// their owners' values, so each rank's rows see the global x0); the step updates owned columns
// only, and the caller keeps the owned ones.
void group_cg_init(Group& G, const double* const* h_b, const double* const* h_x0, const lsq_opts& o, int precond,
                   bool no_stop) {
    std::vector<DBuf<double>> db(G.ranks.size());
    for (size_t r = 0; r < G.ranks.size(); ++r) {
        System& S = *G.ranks[r];
        hipStream_t st = S.stream;
        const Grids lg = grids_for(S);
        db[r].alloc(std::max<int64_t>(S.G.m, 1));
        db[r].upload(h_b[r], S.G.m, st);
        S.cg_x.zero(st);
        S.cg_z.zero(st);
        for (auto& b : S.cg_pb) b.zero(st);
        S.cg_q.zero(st);
        S.cg_s.zero(st);
        if (h_x0) {
            const int64_t n = S.G.n;
            DBuf<double> dx0(std::max<int64_t>(n, 1));
            dx0.upload(h_x0[r], n, st);
            hipLaunchKernelGGL(k_cg_scatter, dim3(grid_for(n)), dim3(BLOCK), 0, st, n, S.keep.p, dx0.p, S.cg_x.p);
            KERNEL_CHECK();
            HIP_CHECK(hipStreamSynchronize(st));   // dx0 is released here
        }
        LsqState ls{};
        HIP_CHECK(hipMemcpyAsync(S.st.p, &ls, sizeof(ls), hipMemcpyHostToDevice, st));
        CgState h{};
        h.atol = o.atol;
        h.btol = o.btol;
        h.maxit = o.maxit > 0 ? o.maxit : INT64_MAX / 4;
        h.no_stop = no_stop ? 1 : 0;
        h.anorm_seed = o.anorm0 > 0.0 ? o.anorm0 : 0.0;
        HIP_CHECK(hipMemcpyAsync(S.cst.p, &h, sizeof(h), hipMemcpyHostToDevice, st));
        S.gsum.zero(st);
        cg_dmf_prepare(S);
        hipLaunchKernelGGL(k_mf_init_u_for(S), dim3(lg.gD + lg.gS), dim3(BLOCK), 0, st, lg.gD, S.mfh.npts, S.Ad.nslices,
                           S.Ad.sp.p, S.Ad.ci.p, S.Ad.val.p, S.Ad.perm.p, S.mfd.p, h_x0 ? S.cg_x.p : nullptr, S.rs.p,
                           db[r].p, S.u.p, S.bw.p, S.part_u.p, S.part_b.p);
        hipLaunchKernelGGL(k_mf_spmtv_for(S), dim3(lg.gM), dim3(BLOCK), 0, st, S.st.p, S.ATd.rp.p, S.ATd.ci.p, S.ATd.val.p,
                           S.mfd.p, S.u.p, S.rs.p, S.csf.p, S.cg_q.p, S.cg_s.p, S.zv.p, S.part_v.p, 1);
        hipLaunchKernelGGL(k_red_parts, dim3(1), dim3(BLOCK), 0, st, S.part_u.p, lg.gD + lg.gS, 0, S.part_b.p,
                           lg.gD + lg.gS, 3, S.gsum.p);
        KERNEL_CHECK();
    }
    group_halo_rev_idx(G, sel_cgs, 0);   // raw Aᵀu of the ghost columns -> their owners
    group_allreduce(G, 0, 4);
    for (System* S : G.ranks)
        hipLaunchKernelGGL(k_cg_init, dim3(1), dim3(BLOCK), 0, S->stream, S->cst.p, S->part_u.p, 0, S->part_b.p, 0,
                           S->gsum.p);
    if (precond == 4) {   // the hierarchy's per-solve set-up, then z0 = V(s0) (α = 0, p = q = 0)
        group_mg_setup(G);
        group_mg_precond(G);
    } else {
        for (System* S : G.ranks)   // α = 0, p = q = 0, pend = 0: z0 = M⁻¹ s0, Σ s0ᵀz0
            cg_launch_precond(*S, cg_grids(*S, precond), precond);
    }
    for (System* S : G.ranks)
        hipLaunchKernelGGL(k_red_parts, dim3(1), dim3(BLOCK), 0, S->stream, S->cg_part_r.p,
                           cg_grids(*S, precond == 4 ? 3 : precond).gB, 6, nullptr, 0, 0, S->gsum.p);
    group_allreduce(G, 6, 1);
    for (System* S : G.ranks) {
        cg_launch_beta(*S, cg_grids(*S, precond), 1);
        S->cg_parity = 0;
    }
    group_halo_fwd_idx(G, sel_cgz, 0);
    KERNEL_CHECK();
    for (System* S : G.ranks) HIP_CHECK(hipStreamSynchronize(S->stream));
}

// the step's partials: [pᵀN_s p, ‖t‖²] after the data rows (precond picks gB through cg_grids:
// 1 and 3 share the normal / data grids), sᵀz after the update
RedSpec red_gam(System& S, int) {
    const CgGrids g = cg_grids(S, 1);
    return {S.cg_part_g.p, g.gN + S.cgh.nedge + S.cg_nvb, 4, S.cg_part_t.p, g.gD, 5};   // + field-valued parts
}
RedSpec red_rho_bj(System& S, int) { return {S.cg_part_r.p, cg_grids(S, 3).gB, 6, nullptr, 0, 0}; }
RedSpec red_rho_jac(System& S, int) { return {S.cg_part_r.p, cg_grids(S, 1).gB, 6, nullptr, 0, 0}; }

void group_cg_iteration(Group& G, int par, int precond) {
    for (System* S : G.ranks) cg_launch_apply(*S, cg_grids(*S, precond), cg_pold(*S, par), cg_pnew(*S, par));
    // partials reduced by the q pack, + all-reduce [pᵀN_s p, ‖t‖²] in the same RCCL group
    group_halo_rev_idx(G, sel_cgq, 0, 4, 2, red_gam);
    for (System* S : G.ranks) {
        const CgGrids g = cg_grids(*S, precond);
        cg_launch_alpha(*S, g);   // from gsum (S.dist)
        if (precond != 4) cg_launch_precond(*S, g, precond);
    }
    if (precond == 4) group_mg_precond(G);
    // sᵀz partials reduced by the z pack; z to the ghosts + all-reduce sᵀz in one RCCL group
    group_halo_fwd_idx(G, sel_cgz, 0, 6, 1, precond == 1 ? red_rho_jac : red_rho_bj);
    for (System* S : G.ranks) cg_launch_beta(*S, cg_grids(*S, precond), 0);
}

// A process-per-GPU rank (one-rank group on RCCL, no device-group fence) replays each batch of
// iterations as a captured hipGraph, RCCL calls included (LSQ_DIST_GRAPH=1; development, off by
// default): the eager path issues ~15 launches per block-Jacobi iteration and ~70 per multigrid one
// from the host.  A capture RCCL or HIP refuses leaves the rank on the eager path.
bool group_cg_graph(Group& G, int count, int precond) {
    static const bool on = getenv("LSQ_DIST_GRAPH") && getenv("LSQ_DIST_GRAPH")[0] == '1';
    System& S0 = *G.ranks[0];
    if (!on || G.virt || G.fence || G.ranks.size() != 1 || count % CG_XK || S0.cg_parity || S0.dist_graph_failed)
        return false;
    GraphCache& c = g_cache_group;
    const int mode = 1000 + precond;
    if (c.exec == nullptr || c.sys != &S0 || c.key != (const void*)S0.cg_x.p || c.batch != count || c.mode != mode) {
        if (c.exec) (void)hipGraphExecDestroy(c.exec);
        c = GraphCache{};
        bool ok = hipStreamBeginCapture(S0.stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            try {
                for (int i = 0; i < count; ++i) {
                    group_cg_iteration(G, S0.cg_parity, precond);
                    S0.cg_parity = (S0.cg_parity + 1) % CG_XK;
                }
            } catch (...) {
                ok = false;
            }
            hipGraph_t graph = nullptr;
            const hipError_t e = hipStreamEndCapture(S0.stream, &graph);
            ok = ok && e == hipSuccess && graph && hipGraphInstantiate(&c.exec, graph, nullptr, nullptr, 0) == hipSuccess;
            if (graph) (void)hipGraphDestroy(graph);
        }
        S0.cg_parity = 0;
        if (!ok) {
            (void)hipGetLastError();
            if (c.exec) (void)hipGraphExecDestroy(c.exec);
            c = GraphCache{};
            S0.dist_graph_failed = true;
            return false;
        }
        c.sys = &S0;
        c.key = S0.cg_x.p;
        c.batch = count;
        c.mode = mode;
    }
    HIP_CHECK(hipGraphLaunch(c.exec, S0.stream));
    return true;
}

void group_cg_run(Group& G, int count, int precond) {
    if (group_cg_graph(G, count, precond)) return;
    for (int i = 0; i < count; ++i) {
        group_cg_iteration(G, G.ranks[0]->cg_parity, precond);
        for (System* S : G.ranks) S->cg_parity = (S->cg_parity + 1) % CG_XK;
    }
    KERNEL_CHECK();
}

// Bytes one rank sends per CG iteration: the step's reverse halo of q and forward halo of z, the
// level-0 operator halos of the V-cycle (2·deg0 operator applications), the partitioned levels'
// row halos (2·deg operator applications with the stencil depth, the restriction's reverse and the
// prolongation's forward halo of one row) and the all-reduce into the first replicated level (a
// ring all-reduce of n doubles sends 2n(N − 1)/N); the scalar all-reduces are not counted.
double group_comm_bytes(const Group& G, int precond) {
    const int N = G.virt ? (int)G.ranks.size() : G.ranks[0]->nranks;
    if (N < 2) return 0.0;
    double worst = 0.0;
    for (const System* S : G.ranks) {
        const double h0 = 8.0 * (double)(S->send_idx.n + S->recv_idx.n);   // one forward + one reverse halo
        double b = h0;
        if (precond == 4 && S->mg) {
            const MgHier& H = *S->mg;
            b += 2.0 * H.deg0 * h0;
            const double ring = 2.0 * (N - 1) / N;
            for (int l = 1; l <= H.lp; ++l) {
                const MgLevel& V = H.lev[l];
                const int sides = (V.oa > 0) + (V.ob < V.geo.S0);
                const int d = std::max(1, std::max(V.tz.hy, V.td.hy));
                b += 8.0 * sides * (2.0 * H.deg * mg_rows_count(V.geo, d) + 2.0 * mg_rows_count(V.geo, 1));
            }
            if (H.lp + 1 < (int)H.lev.size()) b += ring * 8.0 * (double)H.lev[H.lp + 1].geo.n_full;
        }
        worst = std::max(worst, b);
    }
    return worst;
}

void group_cg_stats(Group& G, const CgState& h, int precond, float ms, lsq_stats* stats) {
    if (!stats) return;
    cg_fill_stats(h, stats);
    stats->time_s = ms * 1e-3;
    double b[3];
    cg_kernel_bytes(*G.ranks[0], precond, b);
    stats->bytes_per_iter = b[0] + b[1] + b[2];
    stats->comm_bytes_per_iter = group_comm_bytes(G, precond);
}

}  // namespace

int group_cg_solve(Group& G, const double* const* h_b, double* const* h_x, const lsq_opts& o, lsq_stats* stats) {
    const int precond = o.precond;
    group_cg_prepare(G, precond);
    group_cg_init(G, h_b, o.use_x0 ? h_x : nullptr, o, precond, false);
    const int batch = o.batch > 0 ? o.batch : 16;
    System& S0 = *G.ranks[0];
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, S0.stream));
    CgState h = group_cg_state(G);
    while (!h.stop) {
        group_cg_run(G, batch, precond);
        h = group_cg_state(G);
    }
    for (System* S : G.ranks)   // the owed α p when the last step was not the end of an x cycle
        hipLaunchKernelGGL(k_cg_xfix, dim3(grid_for(S->n_full)), dim3(BLOCK), 0, S->stream, S->cst.p, S->n_full,
                           cg_pbufs(*S), S->cg_x.p);
    HIP_CHECK(hipEventRecord(e1, S0.stream));
    for (size_t r = 0; r < G.ranks.size(); ++r) {   // every local compact column; the caller keeps the owned ones
        System& S = *G.ranks[r];
        const int64_t n = S.G.n;
        DBuf<double> dx(std::max<int64_t>(n, 1));
        hipLaunchKernelGGL(k_cg_gather, dim3(grid_for(n)), dim3(BLOCK), 0, S.stream, n, S.keep.p, S.cg_x.p, dx.p);
        KERNEL_CHECK();
        dx.download(h_x[r], n, S.stream);
        HIP_CHECK(hipStreamSynchronize(S.stream));
        S.cg_ready = false;
    }
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    group_cg_stats(G, h, precond, ms, stats);
    return h.istop == 7 ? 1 : 0;
}

int group_cg_iterate(Group& G, const double* const* h_b, int64_t iters, const lsq_opts& o, lsq_stats* stats) {
    const int precond = o.precond;
    group_cg_prepare(G, precond);
    System& S0 = *G.ranks[0];
    if (!S0.cg_ready || S0.cg_mode != precond) {
        lsq_opts oo = o;
        oo.maxit = INT64_MAX / 4;
        group_cg_init(G, h_b, nullptr, oo, precond, true);
        for (System* S : G.ranks) {
            S->cg_ready = true;
            S->cg_mode = precond;
        }
    }
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, S0.stream));
    group_cg_run(G, (int)iters, precond);
    HIP_CHECK(hipEventRecord(e1, S0.stream));
    const CgState h = group_cg_state(G);
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    group_cg_stats(G, h, precond, ms, stats);
    return 0;
}

// lsq_vgroup_mg_info: what rank r's hierarchy holds after the last multigrid solve — out[0] = levels L,
// out[1] = lp, then per level (λ of the last set-up; 0 for the coarsest, which has no smoother), the
// rank's owned node rows oa, ob (level 0: of the global fine lattice).  Reads state only: no set-up,
// no kernel.  Returns the count written.
int group_mg_info(Group& G, int rank, double* out, int64_t cap) {
    if (rank < 0 || rank >= (int)G.ranks.size()) throw std::invalid_argument("lsq_vgroup_mg_info: rank out of range");
    System& S = *G.ranks[rank];
    if (!S.mg || !S.mg->dist) throw std::invalid_argument("lsq_vgroup_mg_info: no multigrid solve (precond 4) on this group yet");
    const MgHier& H = *S.mg;
    const int64_t L = (int64_t)H.lev.size();
    if (!out || cap < 2 + 3 * L) throw std::invalid_argument("lsq_vgroup_mg_info: output too small");
    std::vector<double> lam((size_t)L, 0.0);
    HIP_CHECK(hipMemcpyAsync(lam.data(), H.lam.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost, S.stream));
    HIP_CHECK(hipStreamSynchronize(S.stream));
    out[0] = (double)L;
    out[1] = (double)H.lp;
    for (int64_t l = 0; l < L; ++l) {
        out[2 + 3 * l] = H.lev[l].coarsest ? 0.0 : lam[l];
        out[3 + 3 * l] = (double)(l ? H.lev[l].oa : H.oa);
        out[4 + 3 * l] = (double)(l ? H.lev[l].ob : H.ob);
    }
    return (int)(2 + 3 * L);
}
