// bias.inc — data biases eliminated from the CGNR normal equations (lsq_set_data_bias).
// Included by lsqr_cg.inc inside its anonymous namespace.
//
// The model gains one additive unknown b_j per bias ID on the data rows (row i carries a 1 in the
// column of its ID) and the constraint rows c_j b_j = 0.  For fixed grid unknowns x the optimal
// b_j = (1/D_j) Σ_{i∈j} W_i² (d_i − (A_d x)_i), D_j = Σ_{i∈j} W_i² + c_j², and substituting it back
// leaves the normal operator N − A_dᵀ W Q W A_d with Q = W B D⁻¹ Bᵀ W.  The CG step already holds
// td_i = W_i² (A_d p)_i per sorted point between k_cg_dmf_ad and k_cg_dmf_atq, so the elimination is
//   s_j = Σ_{i∈j} td_i,   td_i −= W_i² s_j / D_j,   pᵀNp −= Σ_j s_j² / D_j
// on td: a segmented sum by ID (k_bias_chunk, k_bias_seg) and a streaming pass (k_bias_apply).
//
// Reproducibility (BiasData, system.hpp): the points are indexed stably by rank at set time; a wave
// sums one fixed chunk of that index with a segmented shuffle scan and stores one partial per rank it
// touches into that rank's slot of the chunk; k_bias_seg (k_bias_long for the ranks over many chunks)
// then adds each rank's slots in a fixed order.

constexpr int BIAS_E = 8;                     // index entries per lane of a chunk's wave
constexpr int BIAS_CHUNK = 64 * BIAS_E;       // index entries per chunk (one wave)
constexpr int BIAS_LONG = 32;                 // slots above which a rank is summed by a wave of its own

// partial sums of src (per sorted point) by rank, one wave per chunk of the rank-sorted index
__global__ __launch_bounds__(BLOCK) void k_bias_chunk(const CgState* __restrict__ st, int64_t npts, int64_t nchunk,
                                                      const int32_t* __restrict__ idx,
                                                      const int32_t* __restrict__ brank,
                                                      const int32_t* __restrict__ sbase,
                                                      const double* __restrict__ src, double* __restrict__ slots) {
    if (st && st->stop) return;
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (c >= nchunk) return;   // whole waves leave: the shuffles below see full waves
    const int32_t sb = sbase[c];
    const int64_t k0 = c * BIAS_CHUNK + lane;
    int32_t r[BIAS_E], ix[BIAS_E];
    double v[BIAS_E];
#pragma unroll
    for (int e = 0; e < BIAS_E; ++e) {
        const int64_t k = k0 + e * 64;
        r[e] = k < npts ? brank[k] : -1;
        ix[e] = k < npts ? idx[k] : 0;
    }
#pragma unroll
    for (int e = 0; e < BIAS_E; ++e) v[e] = r[e] >= 0 ? src[ix[e]] : 0.0;
    int32_t cr = -1;    // the run that reached the previous trip's last lane, and its sum so far
    double cv = 0.0;
#pragma unroll
    for (int e = 0; e < BIAS_E; ++e) {
        double a = v[e];
        const int32_t rr = r[e];
        if (lane == 0 && cr >= 0) {
            if (cr == rr)
                a = cv + a;
            else
                slots[sb + cr] = cv;
        }
        // segmented inclusive scan: the ranks are sorted, so equal ranks d lanes apart span one run
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double au = __shfl_up(a, d, 64);
            const int32_t ru = __shfl_up(rr, d, 64);
            if (lane >= d && ru == rr) a += au;
        }
        const int32_t rn = __shfl_down(rr, 1, 64);
        if (lane < 63 && rn != rr && rr >= 0) slots[sb + rr] = a;   // the run ends inside this trip
        cr = __shfl(rr, 63, 64);
        cv = __shfl(a, 63, 64);
    }
    if (lane == 0 && cr >= 0) slots[sb + cr] = cv;
}

// the ranks spread over more than BIAS_LONG chunks (listed at set time), a wave each: lane l adds
// the rank's slots l, l + 64, … in chunk order, then the fixed shuffle tree.  Few IDs over many
// points make every rank long; a thread each (k_bias_seg) would add their slots one after the other.
__global__ __launch_bounds__(BLOCK) void k_bias_long(const CgState* __restrict__ st, int64_t nlong,
                                                     const int32_t* __restrict__ long_rank,
                                                     const int32_t* __restrict__ seg,
                                                     const int32_t* __restrict__ sbase,
                                                     const double* __restrict__ slots, double* __restrict__ lsum) {
    if (st && st->stop) return;
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (k >= nlong) return;   // whole waves leave
    const int32_t r = long_rank[k];
    const int32_t ca = seg[r] / BIAS_CHUNK, cb = (seg[r + 1] - 1) / BIAS_CHUNK;
    double t = 0.0;
    for (int32_t c = ca + lane; c <= cb; c += 64) t += slots[sbase[c] + r];
    t = wave_sum(t);
    if (lane == 0) lsum[k] = t;
}

// per rank: the sum of its slots in chunk order.  mode 0: D = Σ + c²; mode 1: sD = Σ / D and, when
// part is given, the workgroup's partial of −Σ_j s_j² / D_j (what the elimination takes off pᵀNp).
// A thread per rank; the long ranks (long_of[r] ≥ 0) take their sum from k_bias_long.
__global__ __launch_bounds__(BLOCK) void k_bias_seg(const CgState* __restrict__ st, int64_t ns,
                                                    const int32_t* __restrict__ seg,
                                                    const int32_t* __restrict__ sbase,
                                                    const double* __restrict__ slots,
                                                    const int32_t* __restrict__ long_of,
                                                    const double* __restrict__ lsum, int mode,
                                                    const double* __restrict__ c2, double* __restrict__ D,
                                                    double* __restrict__ sD, double* part) {
    if (st && st->stop) return;
    double acc = 0.0;
    const int64_t nsp = (ns + BLOCK - 1) / BLOCK * BLOCK;
    for (int64_t r0 = (int64_t)blockIdx.x * BLOCK; r0 < nsp; r0 += (int64_t)gridDim.x * BLOCK) {
        const int64_t r = r0 + threadIdx.x;
        const bool live = r < ns;
        double s = 0.0;
        if (live) {
            const int32_t lo = long_of[r];
            if (lo >= 0) {
                s = lsum[lo];
            } else {
                const int32_t ca = seg[r] / BIAS_CHUNK, cb = (seg[r + 1] - 1) / BIAS_CHUNK;
                for (int32_t c = ca; c <= cb; ++c) s += slots[sbase[c] + r];
            }
        }
        if (live) {
            if (mode == 0) {
                D[r] = s + c2[r];
            } else {
                const double q = s / D[r];
                sD[r] = q;
                acc -= s * q;
            }
        }
    }
    if (part) store_partial(acc, part, blockIdx.x);
}

// mode 0: td −= w² · sD[rank] (the CG step and the cold start); mode 1: td = −w² · sD[rank] (the
// warm start's correction of s0)
__global__ __launch_bounds__(BLOCK) void k_bias_apply(const CgState* __restrict__ st, int64_t npts,
                                                      const int32_t* __restrict__ rank_pt,
                                                      const double* __restrict__ w2, const double* __restrict__ sD,
                                                      double* __restrict__ td, int mode) {
    if (st && st->stop) return;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < npts; i += (int64_t)gridDim.x * BLOCK) {
        const double d = w2[i] * sD[rank_pt[i]];
        td[i] = mode ? -d : td[i] - d;
    }
}

// per solve: w² in sorted point order
__global__ __launch_bounds__(BLOCK) void k_bias_w2(int64_t npts, const int32_t* __restrict__ perm,
                                                   const double* __restrict__ rs, double* __restrict__ w2) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < npts; i += (int64_t)gridDim.x * BLOCK) {
        const double w = rs[perm[i]];
        w2[i] = w * w;
    }
}

// e = w² b − td per sorted point (td = w² A_d x, or null for x = 0): W times the weighted residual
__global__ __launch_bounds__(BLOCK) void k_bias_resid(int64_t npts, const int32_t* __restrict__ perm,
                                                      const double* __restrict__ w2, const double* __restrict__ b,
                                                      const double* td, double* e) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < npts; i += (int64_t)gridDim.x * BLOCK)
        e[i] = w2[i] * b[perm[i]] - (td ? td[i] : 0.0);
}

__global__ __launch_bounds__(BLOCK) void k_bias_scatter(int64_t ns, const int32_t* __restrict__ rank_id,
                                                        const double* __restrict__ sD, double* __restrict__ bval) {
    for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < ns; r += (int64_t)gridDim.x * BLOCK)
        bval[rank_id[r]] = sD[r];
}

// set-time validation: flag bit 0 an ID outside [0, nb), bit 1 a c that is not > 0
__global__ __launch_bounds__(BLOCK) void k_bias_validate(int64_t npts, const int32_t* __restrict__ id, int64_t nb,
                                                         const double* __restrict__ c, int* flag) {
    int f = 0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < npts; i += (int64_t)gridDim.x * BLOCK)
        if (id[i] < 0 || id[i] >= nb) f |= 1;
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < nb; j += (int64_t)gridDim.x * BLOCK)
        if (!(c[j] > 0.0)) f |= 2;
    if (f) atomicOr(flag, f);
}

bool cg_use_dmf(const System& S);

// the biases take part in this system's CGNR operator
inline bool bias_active(const System& S) { return S.bias.on && !S.dist && cg_use_dmf(S); }

// slots = the chunks' partial sums of src by rank
void bias_launch_chunks(const System& S, const CgState* st, const double* src) {
    const BiasData& B = S.bias;
    hipLaunchKernelGGL(k_bias_chunk, dim3((unsigned)((B.nchunk + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0,
                       S.stream, st, B.npts, B.nchunk, B.idx.p, B.brank.p, B.sbase.p, src, B.slots.p);
}

// the slots summed per rank (the long ranks first, a wave each): mode 0 D, mode 1 sD and part
void bias_launch_seg(const System& S, const CgState* st, int mode, double* part) {
    const BiasData& B = S.bias;
    if (B.nlong)
        hipLaunchKernelGGL(k_bias_long, dim3((unsigned)((B.nlong + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0,
                           S.stream, st, B.nlong, B.long_rank.p, B.seg.p, B.sbase.p, B.slots.p, B.lsum.p);
    hipLaunchKernelGGL(k_bias_seg, dim3(B.nbk), dim3(BLOCK), 0, S.stream, st, B.ns, B.seg.p, B.sbase.p, B.slots.p,
                       B.long_of.p, B.lsum.p, mode, B.c2.p, B.D.p, B.sD.p, part);
}

// sD = (Σ_{i∈j} src_i) / D_j per rank; part (nullable): B.nbk partials of −Σ_j s_j² / D_j
void bias_launch_reduce(const System& S, const CgState* st, const double* src, double* part) {
    bias_launch_chunks(S, st, src);
    bias_launch_seg(S, st, 1, part);
}

// the elimination step on td (W² A_d p per sorted point): td ← W (I − Q) W A_d p, part as above
void bias_launch_step(const System& S, const CgState* st, double* td, double* part) {
    const BiasData& B = S.bias;
    bias_launch_reduce(S, st, td, part);
    hipLaunchKernelGGL(k_bias_apply, dim3(grid_for(B.npts)), dim3(BLOCK), 0, S.stream, st, B.npts, B.rank_pt.p, B.w2.p,
                       B.sD.p, td, 0);
}

// per solve (beside k_dmf_rs): w² per sorted point and D_j = Σ w² + c_j² for the current weights / mask
void bias_prepare(System& S) {
    BiasData& B = S.bias;
    hipLaunchKernelGGL(k_bias_w2, dim3(grid_for(B.npts)), dim3(BLOCK), 0, S.stream, B.npts, S.dmf_perm.p, S.rs.p,
                       B.w2.p);
    bias_launch_chunks(S, nullptr, B.w2.p);
    bias_launch_seg(S, nullptr, 0, nullptr);
    KERNEL_CHECK();
}

// algorithmic bytes of one elimination step: the index, the ranks and the gathered td of the chunk
// pass (16 B per point), td read and written, w² and the rank of the apply pass (28 B), the slots
// written and read back with their chunk bases, D and s/D per rank
double bias_step_bytes(const System& S) {
    const BiasData& B = S.bias;
    return 44.0 * (double)B.npts + 20.0 * (double)B.nslots + 4.0 * (double)B.nchunk + 24.0 * (double)B.ns;
}
