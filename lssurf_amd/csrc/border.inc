// border.inc — lsq_cov_band_bordered: error propagation for a banded system with a dense border
// (smooth_fit's data and slope biases: a bias column couples every node its track crosses, so in
// any order the band of the whole AᵀA is the whole matrix).  Included at the end of band.hip.
//
// The z0 / dz columns come first in their band order (n_b of them), the k border columns last:
//
//   AᵀA = [ N   Bᵗ ]     N = R̃ᵀR̃ (band_factor of the principal submatrix, equilibrated by sc)
//         [ B   C  ]     Y = R̃⁻ᵀBᵗ,  S = C − YᵀY = R_SᵀR_S (k × k dense),  V = R̃⁻¹ (Y R_S⁻¹)
//
//   var(band column j)   = (N⁻¹)_jj + ‖V_j·‖²       (the first term: the identity sweeps of band_cov)
//   var(border column j) = ‖(R_S⁻¹)_j·‖²
//   var(op row q, band columns only) = q N⁻¹ qᵀ + ‖q V‖²
//
// all of it on the equilibrated matrix (sc on the band side, s_k = diag(C)^-½ on the border side).
// Bᵗ / Y and Z / V are n_pad × k_pad (k_pad = k rounded up to 64), stored as panels of 64
// right-hand sides: tile (p, K) = rows of band tile K × the 64 columns of panel p, row-major, at
// (p·T + K)·4096.  Y overwrites Bᵗ and V overwrites Z.  One workgroup per panel runs the whole
// forward (backward) substitution: the panels are independent, so there is no grid barrier, and
// every sum has one fixed order (no atomics on doubles): results are bitwise equal run to run.
namespace {

constexpr int BORDER_ROWCAP = 4;   // border entries of one row of A held in registers (k_border_c)

__device__ __forceinline__ double* ptile(double* base, int64_t T, int64_t p, int64_t K) {
    return base + (p * T + K) * TT;
}

// TilePair with a row pitch per tile (a 64×64 block of a dense row-major matrix)
struct TilePairP {
    double2 a[TT / 2 / BLOCK], b[TT / 2 / BLOCK];
    __device__ __forceinline__ void load(const double* pa, int64_t lda, const double* pb, int64_t ldb) {
#pragma unroll
        for (int i = 0; i < TT / 2 / BLOCK; ++i) {
            const int idx = 2 * (threadIdx.x + BLOCK * i), r = idx >> 6, c = idx & 63;
            a[i] = *reinterpret_cast<const double2*>(pa + r * lda + c);
            b[i] = *reinterpret_cast<const double2*>(pb + r * ldb + c);
        }
    }
    __device__ __forceinline__ void store(double* SA, double* SB) const {
#pragma unroll
        for (int i = 0; i < TT / 2 / BLOCK; ++i) {
            const int idx = 2 * (threadIdx.x + BLOCK * i), r = idx >> 6, c = idx & 63;
            SA[r * LDP + c] = a[i].x;
            SA[r * LDP + c + 1] = a[i].y;
            SB[r * LDP + c] = b[i].x;
            SB[r * LDP + c + 1] = b[i].y;
        }
    }
};

// Bᵗ (unscaled): one thread owns band position j (row j of Bᵗ), contributions in the order of
// k_band_normal.  pinv: compact column -> position in the whole order (border: nb + c).
__global__ __launch_bounds__(BLOCK) void k_border_bt(int64_t nb, int64_t T, const int32_t* __restrict__ perm,
                                                     const int32_t* __restrict__ pinv,
                                                     const int64_t* __restrict__ trp, const int32_t* __restrict__ tci,
                                                     const double* __restrict__ tval, const int64_t* __restrict__ rp,
                                                     const int32_t* __restrict__ ci, const double* __restrict__ val,
                                                     const double* __restrict__ rs, double* __restrict__ Bt) {
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < nb; j += (int64_t)gridDim.x * BLOCK) {
        const int64_t K = j >> 6;
        const int rj = (int)(j & 63);
        const int32_t jo = perm[j];
        for (int64_t e = trp[jo]; e < trp[jo + 1]; ++e) {
            const int32_t i = tci[e];
            const double a = tval[e] * rs[i];
            if (a == 0.0) continue;
            for (int64_t f = rp[i]; f < rp[i + 1]; ++f) {
                const int64_t kk = (int64_t)pinv[ci[f]] - nb;
                if (kk < 0) continue;
                ptile(Bt, T, kk >> 6, K)[rj * TB + (kk & 63)] += a * (val[f] * rs[i]);
            }
        }
    }
}

// C (unscaled, upper triangle) and its diagonal: one wave owns border column c and row c of C in
// LDS.  A bias column holds a whole track's rows, so the lanes gather 64 rows of the column at a
// time (each row's border entries at or right of c, in row order), and then add them to the LDS
// row one lane after the other: the order of every sum is the order of the column's rows.
__global__ __launch_bounds__(TB) void k_border_c(int64_t nb, int64_t k, int64_t kpad, const int32_t* __restrict__ perm,
                                                 const int32_t* __restrict__ pinv, const int64_t* __restrict__ trp,
                                                 const int32_t* __restrict__ tci, const double* __restrict__ tval,
                                                 const int64_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                 const double* __restrict__ val, const double* __restrict__ rs,
                                                 double* __restrict__ C, double* __restrict__ dg) {
    extern __shared__ __attribute__((aligned(16))) double crow[];
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x;
    for (int64_t q = lane; q < kpad; q += TB) crow[q] = 0.0;
    __syncthreads();
    const int32_t jo = perm[nb + c];
    const int64_t e1 = trp[jo + 1];
    for (int64_t e0 = trp[jo]; e0 < e1; e0 += TB) {
        const int64_t e = e0 + lane;
        int cnt = 0;
        int32_t kq[BORDER_ROWCAP];
        double pv[BORDER_ROWCAP];
#pragma unroll
        for (int q = 0; q < BORDER_ROWCAP; ++q) {
            kq[q] = 0;
            pv[q] = 0.0;
        }
        int64_t i = -1;
        double a = 0.0;
        if (e < e1) {
            i = tci[e];
            a = tval[e] * rs[i];
            if (a != 0.0)
                for (int64_t f = rp[i]; f < rp[i + 1]; ++f) {
                    const int64_t kk = (int64_t)pinv[ci[f]] - nb;
                    if (kk < c) continue;
                    const double p = a * (val[f] * rs[i]);
#pragma unroll
                    for (int q = 0; q < BORDER_ROWCAP; ++q)
                        if (cnt == q) {
                            kq[q] = (int32_t)kk;
                            pv[q] = p;
                        }
                    ++cnt;
                }
        }
        unsigned long long todo = __ballot(cnt > 0);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            if (lane == l) {
                if (cnt <= BORDER_ROWCAP) {
#pragma unroll
                    for (int q = 0; q < BORDER_ROWCAP; ++q)
                        if (q < cnt) crow[kq[q]] += pv[q];
                } else {   // a row with more border entries than the registers hold: read it again
                    for (int64_t f = rp[i]; f < rp[i + 1]; ++f) {
                        const int64_t kk = (int64_t)pinv[ci[f]] - nb;
                        if (kk >= c) crow[kk] += a * (val[f] * rs[i]);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int64_t q = c + lane; q < k; q += TB) C[c * kpad + q] = crow[q];
    if (lane == 0) dg[c] = crow[c];
}

// s_k = diag(C)^-½ (1 on the padding and for an empty column)
__global__ __launch_bounds__(BLOCK) void k_border_sk(int64_t k, int64_t kpad, const double* __restrict__ dg,
                                                     double* __restrict__ sk) {
    for (int64_t c = (int64_t)blockIdx.x * BLOCK + threadIdx.x; c < kpad; c += (int64_t)gridDim.x * BLOCK) {
        const double d = c < k ? dg[c] : 1.0;
        sk[c] = d > 0.0 ? 1.0 / sqrt(d) : 1.0;
    }
}

// the equilibration: C̃ = s_k C s_k with the identity on the padding, B̃ᵗ = sc Bᵗ s_k
__global__ __launch_bounds__(BLOCK) void k_border_scale(int64_t k, int64_t kpad, int64_t T, const double* __restrict__ sc,
                                                        const double* __restrict__ sk, double* __restrict__ C,
                                                        double* __restrict__ Bt) {
    const int64_t nC = kpad * kpad, nB = (kpad >> 6) * T * TT;
    for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < nC + nB; e += (int64_t)gridDim.x * BLOCK) {
        if (e < nC) {
            const int64_t r = e / kpad, c = e % kpad;
            if (r >= k) C[e] = r == c ? 1.0 : 0.0;
            else C[e] *= sk[r] * sk[c];
        } else {
            const int64_t x = e - nC, tix = x / TT;
            const int idx = (int)(x - tix * TT);
            const int64_t p = tix / T, K = tix % T;
            Bt[x] *= sc[K * TB + (idx >> 6)] * sk[p * TB + (idx & 63)];
        }
    }
}

// Y = R̃⁻ᵀBᵗ in place for the 64 right-hand sides of panel blockIdx.x, tile row by tile row:
// Y_K = D_Kᵀ (Bᵗ_K − Σ_{I=max(0,K−w)}^{K−1} R_IKᵀ Y_I), the scheme of k_band_sweep with dense
// right-hand sides and Y_K stored.  A tile of Y written in one step is read in the next ones
// through global memory: the __threadfence closing each step also invalidates this CU's L1, which
// may hold the tile's lines from when they were Bᵗ.
__global__ __launch_bounds__(BLOCK) void k_border_fsub(BandDev b, double* Y) {
    __shared__ double A[TB * LDP];
    __shared__ double B[TB * LDP];
    double* Yp = Y + (int64_t)blockIdx.x * b.T * TT;
    TilePair tp;
    for (int64_t K = 0; K < b.T; ++K) {
        d4 acc[2][2];
        acc_zero(acc);
        const int64_t I0 = max<int64_t>(0, K - b.w);
        if (I0 < K) tp.load(btile(b.R, b.w, I0, K), Yp + I0 * TT);
        for (int64_t I = I0; I < K; ++I) {
            __syncthreads();
            tp.store(A, B);
            __syncthreads();
            if (I + 1 < K) tp.load(btile(b.R, b.w, I + 1, K), Yp + (I + 1) * TT);
            mma_tile<true>(A, B, acc);
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < TT; idx += BLOCK) {
            const int r = idx >> 6, c = idx & 63;
            B[r * LDP + c] = Yp[K * TT + idx];
            A[r * LDP + c] = b.D[K * TT + idx];
        }
        __syncthreads();
        acc_each(acc, [&](int r, int c, double v) { B[r * LDP + c] -= v; });
        __syncthreads();
        acc_zero(acc);
        mma_tile<true>(A, B, acc);   // D_Kᵀ · X
        double* Yk = Yp + K * TT;
        acc_each(acc, [&](int r, int c, double v) { Yk[r * TB + c] = v; });
        __threadfence();
        __syncthreads();   // the next step's first load reads this tile: every thread's stores have landed
    }
}

// V = R̃⁻¹Z in place, the mirror: V_K = D_K (Z_K − Σ_{J=K+1}^{min(K+w,T−1)} R_KJ V_J), K descending
__global__ __launch_bounds__(BLOCK) void k_border_bsub(BandDev b, double* V) {
    __shared__ double A[TB * LDP];
    __shared__ double B[TB * LDP];
    double* Vp = V + (int64_t)blockIdx.x * b.T * TT;
    TilePair tp;
    for (int64_t K = b.T - 1; K >= 0; --K) {
        d4 acc[2][2];
        acc_zero(acc);
        const int64_t J1 = min<int64_t>(K + b.w, b.T - 1);
        if (K < J1) tp.load(btile(b.R, b.w, K, K + 1), Vp + (K + 1) * TT);
        for (int64_t J = K + 1; J <= J1; ++J) {
            __syncthreads();
            tp.store(A, B);
            __syncthreads();
            if (J + 1 <= J1) tp.load(btile(b.R, b.w, K, J + 1), Vp + (J + 1) * TT);
            mma_tile<false>(A, B, acc);
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < TT; idx += BLOCK) {
            const int r = idx >> 6, c = idx & 63;
            B[r * LDP + c] = Vp[K * TT + idx];
            A[r * LDP + c] = b.D[K * TT + idx];
        }
        __syncthreads();
        acc_each(acc, [&](int r, int c, double v) { B[r * LDP + c] -= v; });
        __syncthreads();
        acc_zero(acc);
        mma_tile<false>(A, B, acc);   // D_K · X
        double* Vk = Vp + K * TT;
        acc_each(acc, [&](int r, int c, double v) { Vk[r * TB + c] = v; });
        __threadfence();
        __syncthreads();
    }
}

// split-K partials of YᵀY: workgroup (p, q ≥ p, s) sums Y(p, K)ᵀ Y(q, K) over its share of the
// tile rows K into part[(s·P + p)·P + q]
__global__ __launch_bounds__(BLOCK) void k_border_syrk(const double* __restrict__ Y, int64_t T, int P, int nsplit,
                                                       double* __restrict__ part) {
    const int p = blockIdx.x, q = blockIdx.y, s = blockIdx.z;
    if (q < p) return;
    __shared__ double A[TB * LDP];
    __shared__ double B[TB * LDP];
    const int64_t Ka = T * s / nsplit, Kb = T * (s + 1) / nsplit;
    const double* Ypp = Y + (int64_t)p * T * TT;
    const double* Yq = Y + (int64_t)q * T * TT;
    d4 acc[2][2];
    acc_zero(acc);
    TilePair tp;
    if (Ka < Kb) tp.load(Ypp + Ka * TT, Yq + Ka * TT);
    for (int64_t K = Ka; K < Kb; ++K) {
        __syncthreads();
        tp.store(A, B);
        __syncthreads();
        if (K + 1 < Kb) tp.load(Ypp + (K + 1) * TT, Yq + (K + 1) * TT);
        mma_tile<true>(A, B, acc);
    }
    double* out = part + (((int64_t)s * P + p) * P + q) * TT;
    acc_each(acc, [&](int r, int c, double v) { out[r * TB + c] = v; });
}

// S = C̃ − YᵀY on the upper tiles, the partials summed in the order of the splits
__global__ __launch_bounds__(BLOCK) void k_border_schur(int P, int nsplit, int64_t kpad, const double* __restrict__ part,
                                                        double* __restrict__ Sm) {
    const int p = blockIdx.x, q = blockIdx.y;
    if (q < p) return;
    for (int idx = threadIdx.x; idx < TT; idx += BLOCK) {
        double sum = 0.0;
        for (int s = 0; s < nsplit; ++s) sum += part[(((int64_t)s * P + p) * P + q) * TT + idx];
        Sm[((int64_t)p * TB + (idx >> 6)) * kpad + (int64_t)q * TB + (idx & 63)] -= sum;
    }
}

// Z = Y·R_S⁻¹ (R_S⁻¹ upper triangular): workgroup (K, q) sums Y(p, K)·Ri[p, q] over p ≤ q
__global__ __launch_bounds__(BLOCK) void k_border_gemm(const double* __restrict__ Y, const double* __restrict__ Ri,
                                                       int64_t T, int64_t kpad, double* __restrict__ Z) {
    __shared__ double A[TB * LDP];
    __shared__ double B[TB * LDP];
    const int64_t K = blockIdx.x;
    const int q = blockIdx.y;
    d4 acc[2][2];
    acc_zero(acc);
    TilePairP tp;
    tp.load(Y + K * TT, TB, Ri + (int64_t)q * TB, kpad);
    for (int p = 0; p <= q; ++p) {
        __syncthreads();
        tp.store(A, B);
        __syncthreads();
        if (p + 1 <= q) tp.load(Y + ((int64_t)(p + 1) * T + K) * TT, TB, Ri + (int64_t)(p + 1) * TB * kpad + (int64_t)q * TB, kpad);
        mma_tile<false>(A, B, acc);
    }
    double* out = Z + ((int64_t)q * T + K) * TT;
    acc_each(acc, [&](int r, int c, double v) { out[r * TB + c] = v; });
}

// Σ_c V[j, c]² per band position j: one wave per row, lane = column within a panel, panels in order
__global__ __launch_bounds__(BLOCK) void k_border_rowss(int64_t nb, int64_t T, int P, const double* __restrict__ V,
                                                        double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < nb; j += (int64_t)gridDim.x * 4) {
        double s = 0.0;
        for (int p = 0; p < P; ++p) {
            const double x = V[((int64_t)p * T + (j >> 6)) * TT + (j & 63) * TB + lane];
            s += x * x;
        }
        s = wave_sum(s);
        if (lane == 0) out[j] = s;
    }
}

// E[perm[j]] = sc_j·sqrt(sweep_j + Σ_c V[j, c]²) on the band, s_k[c]·‖row c of R_S⁻¹‖ on the border
__global__ __launch_bounds__(BLOCK) void k_border_E(int64_t nb, int64_t k, const int32_t* __restrict__ perm,
                                                    const double* __restrict__ ssq, const double* __restrict__ vss,
                                                    const double* __restrict__ sc, const double* __restrict__ rss,
                                                    const double* __restrict__ sk, double* __restrict__ E) {
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < nb + k; j += (int64_t)gridDim.x * BLOCK)
        E[perm[j]] = j < nb ? sqrt(ssq[j] + vss[j]) * sc[j] : rss[j - nb] * sk[j - nb];
}

// ‖q̃ V‖² per op row (q̃ = the row scaled by sc, in band positions): one wave per row
__global__ __launch_bounds__(BLOCK) void k_border_oprows(int64_t nops, const int64_t* __restrict__ rp,
                                                         const int32_t* __restrict__ pos, const double* __restrict__ val,
                                                         const double* __restrict__ sc, int64_t T, int P,
                                                         const double* __restrict__ V, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < nops; i += (int64_t)gridDim.x * 4) {
        double s = 0.0;
        for (int p = 0; p < P; ++p) {
            double t = 0.0;
            for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
                const int64_t j = pos[e];
                t += val[e] * sc[j] * V[((int64_t)p * T + (j >> 6)) * TT + (j & 63) * TB + lane];
            }
            s += t * t;
        }
        s = wave_sum(s);
        if (lane == 0) out[i] = s;
    }
}

}  // namespace

void band_cov_bordered(System& S, const int32_t* h_perm, int64_t nbord, double* h_E, int64_t nops, const int64_t* h_rp,
                       const int32_t* h_ci, const double* h_v, double* h_oe, int64_t* info) {
    hipStream_t st = S.stream;
    const int64_t ncol = S.G.n;
    if (nbord < 1 || nbord > ncol)
        throw std::invalid_argument("lsq_cov_band_bordered: n_border = " + std::to_string(nbord) + " of " +
                                    std::to_string(ncol) + " columns");
    if (nbord > LSQ_BORDER_MAX)
        throw Refused("lsq_cov_band_bordered: a border of " + std::to_string(nbord) + " columns (at most " +
                      std::to_string(LSQ_BORDER_MAX) + ")");
    const int64_t nb = ncol - nbord, k = nbord;
    std::vector<int32_t> pinv(ncol, -1);
    for (int64_t j = 0; j < ncol; ++j) {
        const int32_t o = h_perm[j];
        if (o < 0 || o >= ncol || pinv[o] >= 0)
            throw std::invalid_argument("lsq_cov_band_bordered: perm is not a permutation of the columns");
        pinv[o] = (int32_t)j;
    }
    for (int64_t i = 0; i < nops; ++i)
        for (int64_t e = h_rp[i]; e < h_rp[i + 1]; ++e) {
            if (h_ci[e] < 0 || h_ci[e] >= ncol) throw std::invalid_argument("lsq_cov_band_bordered: op column out of range");
            if (pinv[h_ci[e]] >= nb) throw std::invalid_argument("lsq_cov_band_bordered: an op row reaches a border column");
        }
    const int64_t T = (nb + TB - 1) / TB, npad = T * TB;
    const int64_t kpad = (k + TB - 1) / TB * TB;
    const int P = (int)(kpad / TB);
    const int64_t border_bytes = (2 * npad * kpad + 2 * kpad * kpad) * (int64_t)sizeof(double);
    const auto refuse_mem = [&](int64_t band_bytes, size_t free_b) {
        if ((double)(border_bytes + band_bytes) > 0.8 * ((double)free_b + (double)band_bytes))
            throw Refused("lsq_cov_band_bordered: a border of " + std::to_string(k) + " columns beside " +
                          std::to_string(nb) + " band columns needs " + std::to_string(border_bytes >> 20) +
                          " MiB beside a band of " + std::to_string(band_bytes >> 20) +
                          " MiB, more than the device has free");
    };
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    refuse_mem(0, free_b);   // the border alone, before anything is allocated; with the band once its width is known
    refresh_scaling(S, S.cs_mode < 0 ? 0 : S.cs_mode);
    const auto t0 = std::chrono::steady_clock::now();
    BandFactor F;
    band_factor(S, h_perm, F, nb);
    const auto t1 = std::chrono::steady_clock::now();
    const int w = F.w;
    const int64_t band_bytes = (T * (int64_t)(w + 1) + T) * TT * (int64_t)sizeof(double);
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    refuse_mem(band_bytes, free_b);
    BandDev b{T, w, F.R.p, F.D.p};
    DBuf<double> Y(npad * kpad), Z(npad * kpad), Sm(kpad * kpad), Ri(kpad * kpad);
    DBuf<double> dg(kpad), sk(kpad), vss(npad), rss(kpad);

    // ---- the band's own term, as band_cov: identity sweeps of every tile, then the op rows' sweeps
    const int64_t ring_wg = (int64_t)(w + 1) * TT * (int64_t)sizeof(double);
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const double avail = 0.9 * (double)free_b;
    if (avail < (double)ring_wg * 64)
        throw Refused("lsq_cov_band_bordered: no device memory left for the sweeps of a " + std::to_string(w) +
                      "-tile band");
    const int64_t nop_wg = (nops + TB - 1) / TB;
    const int64_t cap = std::min<int64_t>({(int64_t)(0.5 * avail / ring_wg), std::max(T, nop_wg), 1 << 16});
    DBuf<double> ring(cap * (w + 1) * TT);
    DBuf<double> ssq(npad), dE(ncol);
    run_sweeps<true>(st, b, T, cap, nullptr, nullptr, nullptr, nullptr, nullptr, F.sc.p, ring.p, ssq.p);
    int64_t products = 0;
    for (int64_t J = 0; J < T; ++J) products += (T - J) * (int64_t)std::min<int64_t>(w + 1, T - J);
    std::vector<double> o;
    std::vector<int32_t> opos;
    if (nops > 0) {
        std::vector<int64_t> rows(nops);
        for (int64_t i = 0; i < nops; ++i) rows[i] = i;
        SweepOps so = sweep_ops(rows, h_rp, h_ci, h_v, pinv.data(), T, w);
        products += so.gemms;
        const int64_t nwg = (int64_t)so.sp.size() - 1;
        DBuf<int64_t> dsp(nwg + 1), dsegK((int64_t)so.segK.size()), dsegE((int64_t)so.segE.size());
        DBuf<int32_t> del(std::max<int64_t>((int64_t)so.el.size(), 1));
        DBuf<double> dev(std::max<int64_t>((int64_t)so.ev.size(), 1)), dout(nwg * TB);
        dsp.upload(so.sp.data(), nwg + 1, st);
        dsegK.upload(so.segK.data(), (int64_t)so.segK.size(), st);
        dsegE.upload(so.segE.data(), (int64_t)so.segE.size(), st);
        del.upload(so.el.data(), (int64_t)so.el.size(), st);
        dev.upload(so.ev.data(), (int64_t)so.ev.size(), st);
        run_sweeps<false>(st, b, nwg, cap, dsp.p, dsegK.p, dsegE.p, del.p, dev.p, F.sc.p, ring.p, dout.p);
        o.resize(nwg * TB);
        dout.download(o.data(), nwg * TB, st);
        HIP_CHECK(hipStreamSynchronize(st));
        opos.resize(h_rp[nops]);
        for (int64_t e = 0; e < h_rp[nops]; ++e) opos[e] = pinv[h_ci[e]];
    }
    HIP_CHECK(hipStreamSynchronize(st));
    const auto t2 = std::chrono::steady_clock::now();

    // ---- step 2: Bᵗ and C from the full CSR, equilibrated
    DBuf<int32_t> dperm(ncol), dpinv(ncol);
    dperm.upload(h_perm, ncol, st);
    dpinv.upload(pinv.data(), ncol, st);
    Y.zero(st);
    Sm.zero(st);
    hipLaunchKernelGGL(k_border_bt, dim3(grid_for(nb)), dim3(BLOCK), 0, st, nb, T, dperm.p, dpinv.p, S.GT.rp.p,
                       S.GT.ci.p, S.GT.val.p, S.G.rp.p, S.G.ci.p, S.G.val.p, S.rs.p, Y.p);
    hipLaunchKernelGGL(k_border_c, dim3((unsigned)k), dim3(TB), sizeof(double) * kpad, st, nb, k, kpad, dperm.p, dpinv.p,
                       S.GT.rp.p, S.GT.ci.p, S.GT.val.p, S.G.rp.p, S.G.ci.p, S.G.val.p, S.rs.p, Sm.p, dg.p);
    KERNEL_CHECK();
    hipLaunchKernelGGL(k_border_sk, dim3(grid_for(kpad)), dim3(BLOCK), 0, st, k, kpad, dg.p, sk.p);
    hipLaunchKernelGGL(k_border_scale, dim3(grid_for(kpad * kpad + npad * kpad)), dim3(BLOCK), 0, st, k, kpad, T, F.sc.p,
                       sk.p, Sm.p, Y.p);
    KERNEL_CHECK();
    // ---- step 3: Y = R̃⁻ᵀBᵗ, a workgroup per panel of 64 right-hand sides
    hipLaunchKernelGGL(k_border_fsub, dim3(P), dim3(BLOCK), 0, st, b, Y.p);
    KERNEL_CHECK();
    // ---- step 4: S = C̃ − YᵀY, split-K partials in Z (not yet in use) when they fit there
    int nsplit = (int)std::max<int64_t>(1, std::min<int64_t>({T, T / P, 1024 / ((int64_t)P * P)}));
    DBuf<double> part_own;
    double* part = Z.p;
    if ((int64_t)nsplit * P * P > T * P) {   // a border wider than the band: partials of their own
        part_own.alloc((int64_t)nsplit * P * P * TT);
        part = part_own.p;
    }
    hipLaunchKernelGGL(k_border_syrk, dim3(P, P, nsplit), dim3(BLOCK), 0, st, Y.p, T, P, nsplit, part);
    hipLaunchKernelGGL(k_border_schur, dim3(P, P), dim3(BLOCK), 0, st, P, nsplit, kpad, part, Sm.p);
    KERNEL_CHECK();
    // ---- step 5: S = R_SᵀR_S and R_S⁻¹
    DBuf<int> err(1);
    err.zero(st);
    dense_spd_factor(Sm.p, Ri.p, kpad, err.p, st);
    int h_err = 0;
    HIP_CHECK(hipMemcpyAsync(&h_err, err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (h_err)
        throw std::invalid_argument("lsq_cov_band_bordered: the border block (the Schur complement of the " +
                                    std::to_string(k) + " border columns) is not positive definite: a border "
                                    "column without a kept data row or a weighted constraint row");
    // ---- steps 6, 7: Z = Y·R_S⁻¹, V = R̃⁻¹Z
    hipLaunchKernelGGL(k_border_gemm, dim3((unsigned)T, P), dim3(BLOCK), 0, st, Y.p, Ri.p, T, kpad, Z.p);
    hipLaunchKernelGGL(k_border_bsub, dim3(P), dim3(BLOCK), 0, st, b, Z.p);
    KERNEL_CHECK();
    // ---- step 8
    hipLaunchKernelGGL(k_border_rowss, dim3(grid_for(nb, 4)), dim3(BLOCK), 0, st, nb, T, P, Z.p, vss.p);
    dense_rowrss_of(Ri.p, k, kpad, rss.p, st);
    hipLaunchKernelGGL(k_border_E, dim3(grid_for(ncol)), dim3(BLOCK), 0, st, nb, k, dperm.p, ssq.p, vss.p, F.sc.p, rss.p,
                       sk.p, dE.p);
    KERNEL_CHECK();
    dE.download(h_E, ncol, st);
    if (nops > 0) {
        DBuf<int64_t> drp(nops + 1);
        DBuf<int32_t> dpos(std::max<int64_t>((int64_t)opos.size(), 1));
        DBuf<double> dval(std::max<int64_t>((int64_t)opos.size(), 1)), dadd(nops);
        drp.upload(h_rp, nops + 1, st);
        dpos.upload(opos.data(), (int64_t)opos.size(), st);
        dval.upload(h_v, (int64_t)opos.size(), st);
        hipLaunchKernelGGL(k_border_oprows, dim3(grid_for(nops, 4)), dim3(BLOCK), 0, st, nops, drp.p, dpos.p, dval.p,
                           F.sc.p, T, P, Z.p, dadd.p);
        KERNEL_CHECK();
        std::vector<double> add(nops);
        dadd.download(add.data(), nops, st);
        HIP_CHECK(hipStreamSynchronize(st));
        for (int64_t i = 0; i < nops; ++i) h_oe[i] = std::sqrt(o[i] + add[i]);
    }
    HIP_CHECK(hipStreamSynchronize(st));
    const auto t3 = std::chrono::steady_clock::now();
    if (info) {
        const auto us = [](auto a, auto c) { return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(c - a).count(); };
        int64_t steps = 0;   // tile products of one substitution per panel: Σ_K (min(K, w) + 1)
        for (int64_t K = 0; K < T; ++K) steps += std::min<int64_t>(K, w) + 1;
        info[0] = w;
        info[1] = T;
        info[2] = band_bytes + npad * 16 + ring.n * (int64_t)sizeof(double);
        info[3] = products;
        info[4] = us(t0, t1);   // factor (host wall)
        info[5] = us(t1, t2);   // the band's sweeps
        info[6] = kpad;
        info[7] = border_bytes + (int64_t)part_own.bytes();
        info[8] = us(t2, t3);   // steps 2–8
        info[9] = 2 * (int64_t)P * steps * 2 * TB * TB * TB;   // f64 flops of steps 3 + 7
    }
}
