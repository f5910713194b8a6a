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
//
// Slope biases (lsq_set_data_slope) ride on the same sums with three channels: slope.inc.

constexpr int BIAS_E = 8;                     // index entries per lane of a chunk's wave
constexpr int BIAS_CHUNK = 64 * BIAS_E;       // index entries per chunk (one wave)
constexpr int BIAS_LONG = 32;                 // slots above which a rank is summed by a wave of its own

// One chunk's partial sums of NCH channels by rank: src, and with three channels src·u₀ and src·u₁
// (slope.inc).  Channel ch stores into plane ch of the slots (plane = nslots doubles).  The
// one-channel instantiation is the sum the biases always ran, operation for operation.
template <int NCH>
__device__ __forceinline__ void bias_chunk_sum(int lane, int64_t npts, int64_t c, int32_t sb,
                                               const int32_t* __restrict__ idx, const int32_t* __restrict__ brank,
                                               const double* __restrict__ src, const double2* __restrict__ u,
                                               double* __restrict__ slots, int64_t nslots) {
    const int64_t k0 = c * BIAS_CHUNK + lane;
    int32_t r[BIAS_E], ix[BIAS_E];
    double v[BIAS_E][NCH];
#pragma unroll
    for (int e = 0; e < BIAS_E; ++e) {
        const int64_t k = k0 + e * 64;
        r[e] = k < npts ? brank[k] : -1;
        ix[e] = k < npts ? idx[k] : 0;
    }
#pragma unroll
    for (int e = 0; e < BIAS_E; ++e) {
        v[e][0] = r[e] >= 0 ? src[ix[e]] : 0.0;
        if (NCH > 1) {
            const double2 uu = r[e] >= 0 ? u[ix[e]] : make_double2(0.0, 0.0);
            v[e][1 % NCH] = v[e][0] * uu.x;
            v[e][2 % NCH] = v[e][0] * uu.y;
        }
    }
    int32_t cr = -1;    // the run that reached the previous trip's last lane, and its sums so far
    double cv[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) cv[ch] = 0.0;
#pragma unroll
    for (int e = 0; e < BIAS_E; ++e) {
        double a[NCH];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) a[ch] = v[e][ch];
        const int32_t rr = r[e];
        if (lane == 0 && cr >= 0) {
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                if (cr == rr)
                    a[ch] = cv[ch] + a[ch];
                else
                    slots[ch * nslots + sb + cr] = cv[ch];
            }
        }
        // segmented inclusive scan: the ranks are sorted, so equal ranks d lanes apart span one run
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t ru = __shfl_up(rr, d, 64);
            const bool take = lane >= d && ru == rr;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const double au = __shfl_up(a[ch], d, 64);
                if (take) a[ch] += au;
            }
        }
        const int32_t rn = __shfl_down(rr, 1, 64);
        if (lane < 63 && rn != rr && rr >= 0) {   // the run ends inside this trip
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) slots[ch * nslots + sb + rr] = a[ch];
        }
        cr = __shfl(rr, 63, 64);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) cv[ch] = __shfl(a[ch], 63, 64);
    }
    if (lane == 0 && cr >= 0) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) slots[ch * nslots + sb + cr] = cv[ch];
    }
}

// partial sums of src (per sorted point) by rank, one wave per chunk of the rank-sorted index.
// NCH = 3 (slopes set): the chunks that start at a rank inside a slope group (rank < nsr) sum the
// three channels, the others the first only.
template <int NCH>
__global__ __launch_bounds__(BLOCK) void k_bias_chunk(const CgState* __restrict__ st, int64_t npts, int64_t nchunk,
                                                      const int32_t* __restrict__ idx,
                                                      const int32_t* __restrict__ brank,
                                                      const int32_t* __restrict__ sbase,
                                                      const double* __restrict__ src, double* __restrict__ slots,
                                                      const double2* __restrict__ u, int64_t nslots, int32_t nsr) {
    if (st && st->stop) return;
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (c >= nchunk) return;   // whole waves leave: the shuffles below see full waves
    const int32_t sb = sbase[c];
    if (NCH > 1 && brank[c * BIAS_CHUNK] >= nsr)   // wave-uniform: no rank of this chunk lies in a group
        bias_chunk_sum<1>(lane, npts, c, sb, idx, brank, src, u, slots, nslots);
    else
        bias_chunk_sum<NCH>(lane, npts, c, sb, idx, brank, src, u, slots, nslots);
}

// the ranks spread over more than BIAS_LONG chunks (listed at set time), a wave each: lane l adds
// the rank's slots l, l + 64, … in chunk order, then the fixed shuffle tree.  Few IDs over many
// points make every rank long; a thread each (k_bias_seg) would add their slots one after the other.
// NCH = 3: the ranks below nsr sum their three planes into the three planes of lsum.
template <int NCH>
__global__ __launch_bounds__(BLOCK) void k_bias_long(const CgState* __restrict__ st, int64_t nlong,
                                                     const int32_t* __restrict__ long_rank,
                                                     const int32_t* __restrict__ seg,
                                                     const int32_t* __restrict__ sbase,
                                                     const double* __restrict__ slots, double* __restrict__ lsum,
                                                     int64_t nslots, int32_t nsr) {
    if (st && st->stop) return;
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (k >= nlong) return;   // whole waves leave
    const int32_t r = long_rank[k];
    const int32_t ca = seg[r] / BIAS_CHUNK, cb = (seg[r + 1] - 1) / BIAS_CHUNK;
    const int nch = NCH > 1 && r < nsr ? NCH : 1;
    for (int ch = 0; ch < nch; ++ch) {
        double t = 0.0;
        for (int32_t c = ca + lane; c <= cb; c += 64) t += slots[ch * nslots + sbase[c] + r];
        t = wave_sum(t);
        if (lane == 0) lsum[ch * nlong + k] = t;
    }
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

#include "slope.inc"

bool cg_use_dmf(const System& S);

// the biases (and slopes) take part in this system's CGNR operator
inline bool bias_active(const System& S) { return S.bias.on && !S.dist && cg_use_dmf(S); }

// slots = the chunks' partial sums of src by rank (slopes set: three channels where a group lies)
void bias_launch_chunks(const System& S, const CgState* st, const double* src) {
    const BiasData& B = S.bias;
    const dim3 grid((unsigned)((B.nchunk + BLOCK / 64 - 1) / (BLOCK / 64)));
    const double2* u = reinterpret_cast<const double2*>(B.u.p);
    if (B.ng)
        hipLaunchKernelGGL(k_bias_chunk<3>, grid, dim3(BLOCK), 0, S.stream, st, B.npts, B.nchunk, B.idx.p, B.brank.p,
                           B.sbase.p, src, B.slots.p, u, B.nslots, (int32_t)B.nsr);
    else
        hipLaunchKernelGGL(k_bias_chunk<1>, grid, dim3(BLOCK), 0, S.stream, st, B.npts, B.nchunk, B.idx.p, B.brank.p,
                           B.sbase.p, src, B.slots.p, u, B.nslots, 0);
}

// the slots summed per rank (the long ranks first, a wave each): mode 0 D, mode 1 sD and part.
// Slopes set: the ranks' channel sums into rsum; mode 1 also β of the ranks outside every group
void bias_launch_seg(const System& S, const CgState* st, int mode, double* part) {
    const BiasData& B = S.bias;
    const dim3 gl((unsigned)((B.nlong + BLOCK / 64 - 1) / (BLOCK / 64)));
    if (B.ng) {
        if (B.nlong)
            hipLaunchKernelGGL(k_bias_long<3>, gl, dim3(BLOCK), 0, S.stream, st, B.nlong, B.long_rank.p, B.seg.p,
                               B.sbase.p, B.slots.p, B.lsum.p, B.nslots, (int32_t)B.nsr);
        hipLaunchKernelGGL(k_slope_rank, dim3(B.nrk), dim3(BLOCK), 0, S.stream, st, B.ns, (int32_t)B.nsr, B.seg.p,
                           B.sbase.p, B.slots.p, B.nslots, B.long_of.p, B.lsum.p, B.nlong, mode, (int)B.pseudo, B.D.p,
                           B.rsum.p, B.sD.p, part);
        return;
    }
    if (B.nlong)
        hipLaunchKernelGGL(k_bias_long<1>, gl, dim3(BLOCK), 0, S.stream, st, B.nlong, B.long_rank.p, B.seg.p,
                           B.sbase.p, B.slots.p, B.lsum.p, B.nslots, 0);
    hipLaunchKernelGGL(k_bias_seg, dim3(B.nbk), dim3(BLOCK), 0, S.stream, st, B.ns, B.seg.p, B.sbase.p, B.slots.p,
                       B.long_of.p, B.lsum.p, mode, B.c2.p, B.D.p, B.sD.p, part);
}

// a wave per slope group over the ranks' channel sums (k_slope_group's modes)
void slope_launch_group(const System& S, const CgState* st, int mode, double* part) {
    const BiasData& B = S.bias;
    hipLaunchKernelGGL(k_slope_group, dim3(B.ngk), dim3(BLOCK), 0, S.stream, st, B.ng, B.ns, B.gseg.p, mode,
                       (int)B.pseudo, B.rsum.p, B.D.p, B.e.p, B.gc2.p, B.F.p, B.L.p, B.gam.p, B.sD.p, part);
}

// sD = β per rank for the sums of src: (Σ_{i∈j} src_i) / D_j, and with slopes γ per group and
// β_j = (s_j − e_j·γ) / D_j.  part (nullable): B.nbk partials of −(Σ_j s_j β_j + Σ_s h_s·γ_s).
// marks (nullable): the step's stages E0 (chunk pass), E1 (per-rank sums), E2 (per-group kernel)
void bias_launch_reduce(const System& S, const CgState* st, const double* src, double* part, CgMarks* marks = nullptr) {
    bias_launch_chunks(S, st, src);
    cg_mark(marks, CG_E0, S.stream);
    bias_launch_seg(S, st, 1, part);
    cg_mark(marks, CG_E1, S.stream);
    if (S.bias.ng) slope_launch_group(S, st, 2, part ? part + S.bias.nrk : nullptr);
    cg_mark(marks, CG_E2, S.stream);
}

// mode 0: td −= W² Z [β; γ]; mode 1: td = −W² Z [β; γ] (after bias_launch_reduce)
void bias_launch_apply(const System& S, const CgState* st, double* td, int mode) {
    const BiasData& B = S.bias;
    if (B.ng)
        hipLaunchKernelGGL(k_slope_apply, dim3(grid_for(B.npts)), dim3(BLOCK), 0, S.stream, st, B.npts, (int32_t)B.nsr,
                           B.rank_pt.p, B.rgrp.p, B.w2.p, B.sD.p, reinterpret_cast<const double2*>(B.u.p), B.gam.p, td,
                           mode);
    else
        hipLaunchKernelGGL(k_bias_apply, dim3(grid_for(B.npts)), dim3(BLOCK), 0, S.stream, st, B.npts, B.rank_pt.p,
                           B.w2.p, B.sD.p, td, mode);
}

// per solve (beside k_dmf_rs): w² per sorted point and D_j = Σ w² + c_j² for the current weights / mask;
// slopes set: also e_j, F_s and the Cholesky factor of G_s (three passes: over w², w² u₀, w² u₁)
void bias_prepare(System& S) {
    BiasData& B = S.bias;
    hipLaunchKernelGGL(k_bias_w2, dim3(grid_for(B.npts)), dim3(BLOCK), 0, S.stream, B.npts, S.dmf_perm.p, S.rs.p,
                       B.w2.p);
    bias_launch_chunks(S, nullptr, B.w2.p);
    bias_launch_seg(S, nullptr, 0, nullptr);
    if (B.ng) {
        hipLaunchKernelGGL(k_slope_de, dim3(grid_for(B.ns)), dim3(BLOCK), 0, S.stream, B.ns, (int32_t)B.nsr,
                           (int)B.pseudo, B.rsum.p, B.c2.p, B.D.p, B.e.p);
        for (int k = 0; k < 2; ++k) {
            hipLaunchKernelGGL(k_slope_w2u, dim3(grid_for(B.npts)), dim3(BLOCK), 0, S.stream, B.npts, B.w2.p,
                               reinterpret_cast<const double2*>(B.u.p), k, B.tmp.p);
            bias_launch_chunks(S, nullptr, B.tmp.p);
            bias_launch_seg(S, nullptr, 0, nullptr);
            slope_launch_group(S, nullptr, k, nullptr);
        }
    }
    KERNEL_CHECK();
}

// Slopes set: algorithmic bytes of the step's kernels, out = {chunk pass, per-rank sums (with the
// long ranks' kernel), per-group kernel, apply pass}.  Chunk pass: the index, the ranks and the
// gathered td (16 B per point), u in the three-channel chunks (16 B), the slots written (three planes
// where a group lies) and the chunk bases.  Per rank: the slots read back with their chunk bases, the
// sums written (three below nsr), D read and β written outside the groups.  Per group: its ranks' three
// sums, D and e read and β written, L read and γ written.  Apply: td read and written, w² and the rank
// (28 B per point), u on the rows of the three-channel chunks (16 B).
void slope_kernel_bytes(const System& S, double out[4]) {
    const BiasData& B = S.bias;
    const double np = (double)B.npts, np3 = (double)B.npts3, sl = (double)B.nslots, sl3 = (double)B.nslots3;
    const double ns = (double)B.ns, nsr = (double)B.nsr, ng = (double)B.ng;
    out[0] = 16.0 * np + 16.0 * np3 + 8.0 * sl + 16.0 * sl3 + 4.0 * (double)B.nchunk;
    out[1] = 12.0 * sl + 16.0 * sl3 + 8.0 * ns + 16.0 * nsr + 16.0 * (ns - nsr);
    out[2] = 56.0 * nsr + 40.0 * ng;
    out[3] = 28.0 * np + 16.0 * np3;
}

// algorithmic bytes of one elimination step: the index, the ranks and the gathered td of the chunk
// pass (16 B per point), td read and written, w² and the rank of the apply pass (28 B), the slots
// written and read back with their chunk bases, D and s/D per rank.  Slopes set: the sum of
// slope_kernel_bytes
double bias_step_bytes(const System& S) {
    const BiasData& B = S.bias;
    if (B.ng) {
        double k[4];
        slope_kernel_bytes(S, k);
        return k[0] + k[1] + k[2] + k[3];
    }
    return 44.0 * (double)B.npts + 20.0 * (double)B.nslots + 4.0 * (double)B.nchunk + 24.0 * (double)B.ns;
}
