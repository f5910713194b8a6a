// bsolve.inc — lsq_cov_border_solved: the border term of compute_E at window scale (smooth_fit's data
// and slope biases beside tiled windows, lssurf_amd/errors.py).  Included at the end of lsqr.hip.
//
// The handle holds the grid-only system A_g (its weights W = row weight × mask); the caller passes the
// k border columns B of the data rows (CSC, unweighted) and c_con, the weighted share of C from rows
// that touch border columns only.  With
//
//   AᵀA = [ N  Bᵗ ]   N = A_gᵀW²A_g,   C = BᵗW²B + c_con,   Z = N⁻¹ A_gᵀ W² B  (n × k)
//         [ B  C  ]   S = C − ½(T + Tᵀ),  T = BᵗW²A_d Z  (= BN⁻¹Bᵗ, symmetric for exact solves)
//
//   var_add[j]    = ‖V_j·‖²,  V = Z s_k R̃_S⁻¹,   S̃ = s_k S s_k = R̃_SᵀR̃_S,  s_k = diag(C)^-½
//   var_border[j] = s_k[j]² ‖(R̃_S⁻¹)_j·‖²
//   op_add[i]     = ‖(op_i Z) s_k R̃_S⁻¹‖²
//
// border.inc gets N⁻¹Bᵗ from the band factor of N; here column j of Z is one CGNR solve of the
// grid-only system with column j of B as the right-hand side: x = argmin ‖W(A_g x − b_j)‖ = N⁻¹A_gᵀW²b_j.
// Z is n_pad × k_pad column-major (n_pad, k_pad: n, k rounded up to 64).  Nothing of length n or m
// crosses to the host between the steps; every sum has one fixed order (no atomics on doubles), so a
// second call returns the same bits.
namespace {

constexpr int BS_TB = 64;
constexpr int BS_TT = BS_TB * BS_TB;
constexpr int BS_LDP = BS_TB + 1;   // LDS tile pitch
typedef double bs_d4 __attribute__((ext_vector_type(4)));

// step 2: column j of B into the right-hand side (the data rows were zeroed)
__global__ __launch_bounds__(BLOCK) void k_bs_scatter(int64_t e0, int64_t e1, const int32_t* __restrict__ rows,
                                                      const double* __restrict__ vals, double* __restrict__ b) {
    for (int64_t e = e0 + (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < e1; e += (int64_t)gridDim.x * BLOCK)
        b[rows[e]] = vals[e];
}

// out[c] = Σ_{rows r of border column c, in row order} (B[r, c]·y[r])·rs[r]²: one wave per border column,
// lane l sums the entries l, l + 64, … of the column, then the wave's butterfly: one fixed order.
// y = column j of B (C[:, j]) or A_d z_j (T[:, j]).
__global__ __launch_bounds__(WAVE) void k_bs_gather(const int64_t* __restrict__ cp, const int32_t* __restrict__ rows,
                                                    const double* __restrict__ vals, const double* __restrict__ rs,
                                                    const double* __restrict__ y, double* __restrict__ out) {
    const int64_t c = blockIdx.x;
    double s = 0.0;
    for (int64_t e = cp[c] + threadIdx.x; e < cp[c + 1]; e += WAVE) {
        const int32_t r = rows[e];
        const double w = rs[r];
        s += (vals[e] * y[r]) * (w * w);
    }
    s = wave_sum(s);
    if (threadIdx.x == 0) out[c] = s;
}

// s_k = (C_cc + c_con_cc)^-½ (1 on the padding and for a diagonal that is not positive)
__global__ __launch_bounds__(BLOCK) void k_bs_sk(int64_t k, int64_t kpad, const double* __restrict__ C,
                                                 const double* __restrict__ ccon, double* __restrict__ sk) {
    for (int64_t c = (int64_t)blockIdx.x * BLOCK + threadIdx.x; c < kpad; c += (int64_t)gridDim.x * BLOCK) {
        const double d = c < k ? C[c * kpad + c] + ccon[c * k + c] : 1.0;
        sk[c] = d > 0.0 ? 1.0 / sqrt(d) : 1.0;
    }
}

// S̃ = s_k (C + c_con − ½(T + Tᵀ)) s_k in place of C (row p per workgroup; the identity on the padding)
// and asym[p] = max_q |T_pq − T_qp| s_p s_q
__global__ __launch_bounds__(BLOCK) void k_bs_schur(int64_t k, int64_t kpad, const double* __restrict__ ccon,
                                                    const double* __restrict__ T, const double* __restrict__ sk,
                                                    double* __restrict__ Sm, double* __restrict__ asym) {
    __shared__ double red[BLOCK];
    const int64_t p = blockIdx.x;
    double a = 0.0;
    for (int64_t q = threadIdx.x; q < kpad; q += BLOCK) {
        double v = p == q ? 1.0 : 0.0;
        if (p < k && q < k) {
            const double t1 = T[p * kpad + q], t2 = T[q * kpad + p], s = sk[p] * sk[q];
            v = (Sm[p * kpad + q] + ccon[p * k + q] - 0.5 * (t1 + t2)) * s;
            a = fmax(a, fabs(t1 - t2) * s);
        }
        Sm[p * kpad + q] = v;
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) asym[p] = red[0];
}

// Ri ← s_k Ri (rows), rss[p] = Σ_q Ri[p, q]² (one wave per row, lanes strided over the columns, butterfly),
// piv[p] = R[p, p]² (the pivots of the equilibrated S)
__global__ __launch_bounds__(WAVE) void k_bs_ri(int64_t kpad, const double* __restrict__ R, const double* __restrict__ sk,
                                                double* __restrict__ Ri, double* __restrict__ rss,
                                                double* __restrict__ piv) {
    const int64_t p = blockIdx.x;
    const double s = sk[p];
    double ss = 0.0;
    for (int64_t q = p - (p & 63) + threadIdx.x; q < kpad; q += WAVE) {
        const double v = q >= p ? Ri[p * kpad + q] * s : 0.0;
        Ri[p * kpad + q] = v;
        ss += v * v;
    }
    ss = wave_sum(ss);
    if (threadIdx.x == 0) {
        rss[p] = ss;
        const double d = R[p * kpad + p];
        piv[p] = d * d;
    }
}

// step 5: out[r] = Σ_q (Σ_{p ≤ q} X[r, p] Ri[p, q])² for the 64 rows of panel blockIdx.x of X (ld × kpad,
// column-major: Z, or op·Z), Ri upper triangular kpad × kpad row-major.  Per column tile q the
// workgroup sums X(panel, p)·Ri(p, q) over the tiles p ≤ q (the zero tiles of the triangle are
// skipped) on v_mfma_f64_16x16x4_f64 — wave wv owns the 32 × 32 block (r0, c0) as 2 × 2 accumulators,
// element (s, t, g) = row r0 + 16s + (lane>>4) + 4g, column c0 + 16t + (lane&15) — and adds the squares
// to its rows' partial sums; V itself is never stored.  The X tile lands in LDS as [k][row] (its
// global layout: 64 contiguous rows per column), the Ri tile as [k][col]: both MFMA operand reads walk
// consecutive lanes along a row of the image.  The next tile pair's loads are in flight while the
// MFMAs of the current one run.  The row sums close in a fixed order: 32 slots per row in LDS (wave
// column half × lane&15), summed by one thread per row.
struct BsPair {
    double2 a[BS_TT / 2 / BLOCK], b[BS_TT / 2 / BLOCK];
    __device__ __forceinline__ void load(const double* __restrict__ pa, int64_t lda, const double* __restrict__ pb,
                                         int64_t ldb) {
#pragma unroll
        for (int i = 0; i < BS_TT / 2 / BLOCK; ++i) {
            const int idx = 2 * (threadIdx.x + BLOCK * i), r = idx >> 6, c = idx & 63;
            a[i] = *reinterpret_cast<const double2*>(pa + r * lda + c);
            b[i] = *reinterpret_cast<const double2*>(pb + r * ldb + c);
        }
    }
    __device__ __forceinline__ void store(double* SA, double* SB) const {
#pragma unroll
        for (int i = 0; i < BS_TT / 2 / BLOCK; ++i) {
            const int idx = 2 * (threadIdx.x + BLOCK * i), r = idx >> 6, c = idx & 63;
            SA[r * BS_LDP + c] = a[i].x;
            SA[r * BS_LDP + c + 1] = a[i].y;
            SB[r * BS_LDP + c] = b[i].x;
            SB[r * BS_LDP + c + 1] = b[i].y;
        }
    }
};

__global__ __launch_bounds__(BLOCK) void k_bs_vss(const double* __restrict__ X, int64_t ld, int64_t kpad,
                                                  const double* __restrict__ Ri, double* __restrict__ out) {
    __shared__ double A[BS_TB * BS_LDP];   // [k][row]
    __shared__ double B[BS_TB * BS_LDP];   // [k][col]
    const int P = (int)(kpad / BS_TB);
    const double* Xp = X + (int64_t)blockIdx.x * BS_TB;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r0 = (wv >> 1) * 32, c0 = (wv & 1) * 32;
    const int li = lane & 15, lk = lane >> 4;
    double rsum[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int g = 0; g < 4; ++g) rsum[s][g] = 0.0;
    BsPair tp;
    tp.load(Xp, ld, Ri, kpad);   // (p, q) = (0, 0)
    for (int q = 0; q < P; ++q) {
        bs_d4 acc[2][2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[s][t] = bs_d4{0.0, 0.0, 0.0, 0.0};
        for (int p = 0; p <= q; ++p) {
            __syncthreads();
            tp.store(A, B);
            __syncthreads();
            const int pn = p < q ? p + 1 : 0, qn = p < q ? q : q + 1;   // the next pair in this order
            if (qn < P)
                tp.load(Xp + (int64_t)pn * BS_TB * ld, ld, Ri + (int64_t)pn * BS_TB * kpad + (int64_t)qn * BS_TB, kpad);
#pragma unroll 4
            for (int k0 = 0; k0 < BS_TB; k0 += 4) {
                const int kk = k0 + lk;
                const double a0 = A[kk * BS_LDP + r0 + li], a1 = A[kk * BS_LDP + r0 + 16 + li];
                const double b0 = B[kk * BS_LDP + c0 + li], b1 = B[kk * BS_LDP + c0 + 16 + li];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const double v0 = acc[s][0][g], v1 = acc[s][1][g];
                rsum[s][g] += v0 * v0 + v1 * v1;
            }
    }
    __syncthreads();   // the last pair's MFMA reads of A are done: A becomes the 64 × 32 slots
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int g = 0; g < 4; ++g) A[(r0 + 16 * s + lk + 4 * g) * 32 + (wv & 1) * 16 + li] = rsum[s][g];
    __syncthreads();
    if (threadIdx.x < BS_TB) {
        double s = 0.0;
        for (int i = 0; i < 32; ++i) s += A[threadIdx.x * 32 + i];
        out[(int64_t)blockIdx.x * BS_TB + threadIdx.x] = s;
    }
}

// step 6: XZ = op·Z for the op rows [i0, i0 + cnt) (compact columns), column-major ldo × kpad: one wave
// per op row, lane = column of a 64-column tile, the row's entries in their order
__global__ __launch_bounds__(BLOCK) void k_bs_opz(int64_t i0, int64_t cnt, const int64_t* __restrict__ rp,
                                                  const int32_t* __restrict__ ci, const double* __restrict__ val,
                                                  const double* __restrict__ Z, int64_t npad, int64_t kpad, int64_t ldo,
                                                  double* __restrict__ XZ) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < cnt; i += (int64_t)gridDim.x * 4) {
        const int64_t ea = rp[i0 + i], eb = rp[i0 + i + 1];
        for (int64_t c = lane; c < kpad; c += 64) {
            double t = 0.0;
            for (int64_t e = ea; e < eb; ++e) t += val[e] * Z[c * npad + ci[e]];
            XZ[c * ldo + i] = t;
        }
    }
}

int64_t bs_need_bytes(int64_t npad, int64_t kpad) { return (npad * kpad + 3 * kpad * kpad) * (int64_t)sizeof(double); }

}  // namespace

// Returns 0, or −1 with S.err set when a column's solve did not converge (no output is written).
// info (12): k_pad, device bytes of Z and the three k_pad² blocks, total and largest CG iterations of
// a column, µs of the solves, of steps 3, 4, 5 and 6 (host wall clock around a synchronised stream),
// asym, the smallest pivot of the equilibrated S, µs of the step-5 kernel on Z alone (device events).
int cov_border_solved(System& S, int64_t k, const int64_t* h_cp, const int32_t* h_rows, const double* h_vals,
                      const double* h_ccon, const lsq_opts& o, int64_t nops, const int64_t* h_rp, const int32_t* h_ci,
                      const double* h_v, double* h_var_add, double* h_var_border, double* h_op_add, double* info) {
    const char* who = "lsq_cov_border_solved: ";
    hipStream_t st = S.stream;
    if (S.dist) throw std::invalid_argument(std::string(who) + "the handle is a rank of a group (single-GPU handles only)");
    if (S.bias.nb || S.bias.ng || S.sgrid.ng)
        throw std::invalid_argument(std::string(who) + "a bias, slope or sensor-grid elimination is set on the handle: the "
                                    "border columns are passed to this call, the handle holds the grid-only system");
    if (k < 1) throw std::invalid_argument(std::string(who) + "k = " + std::to_string(k) + " border columns");
    if (k > LSQ_BORDER_MAX)
        throw Refused(std::string(who) + "a border of " + std::to_string(k) + " columns (at most " +
                      std::to_string(LSQ_BORDER_MAX) + ")");
    const int precond = o.precond;
    if (precond != 1 && precond != 3 && precond != 4)
        throw std::invalid_argument(std::string(who) + "the solves run as CGNR with precond 1 (Jacobi), 3 (block-Jacobi) "
                                    "or 4 (multigrid), not " + std::to_string(precond));
    if (S.xr.m_x) {
        const std::string why = xr_refusal(S, 1, precond, 0);
        if (!why.empty()) throw std::invalid_argument(who + why);
    }
    if (!cg_available(S, precond))   // builds the row scales, the block factors and the levels when stale
        throw std::invalid_argument(std::string(who) + "no CGNR operator for precond " + std::to_string(precond) + ": " +
                                    (S.cg_ok ? S.mg_why : S.cg_why.empty() ? "not a structured single-GPU system" : S.cg_why));
    const int64_t n = S.G.n, m = S.G.m, npts = S.mfh.npts;
    if (h_cp[0] != 0) throw std::invalid_argument(std::string(who) + "colptr[0] must be 0");
    for (int64_t c = 0; c < k; ++c) {
        if (h_cp[c + 1] < h_cp[c]) throw std::invalid_argument(std::string(who) + "colptr must not decrease");
        for (int64_t e = h_cp[c]; e < h_cp[c + 1]; ++e) {
            if (h_rows[e] < 0 || h_rows[e] >= npts)
                throw std::invalid_argument(std::string(who) + "border column " + std::to_string(c) + " holds row " +
                                            std::to_string(h_rows[e]) + " outside the " + std::to_string(npts) + " data rows");
            if (e > h_cp[c] && h_rows[e] <= h_rows[e - 1])
                throw std::invalid_argument(std::string(who) + "the rows of border column " + std::to_string(c) +
                                            " must be strictly increasing");
            if (!std::isfinite(h_vals[e]))
                throw std::invalid_argument(std::string(who) + "border column " + std::to_string(c) + " holds a value that is not finite");
        }
    }
    for (int64_t e = 0; e < k * k; ++e)
        if (!std::isfinite(h_ccon[e])) throw std::invalid_argument(std::string(who) + "c_con holds a value that is not finite");
    for (int64_t i = 0; i < nops; ++i) {
        if (h_rp[i + 1] < h_rp[i]) throw std::invalid_argument(std::string(who) + "op_ptr must not decrease");
        for (int64_t e = h_rp[i]; e < h_rp[i + 1]; ++e)
            if (h_ci[e] < 0 || h_ci[e] >= n) throw std::invalid_argument(std::string(who) + "op column out of range");
    }
    const int64_t nnzb = h_cp[k];
    const int64_t npad = (n + BS_TB - 1) / BS_TB * BS_TB, kpad = (k + BS_TB - 1) / BS_TB * BS_TB;
    // ---- the byte budget, before anything of the border is allocated (LSQ_BSOLVE_BUDGET: development
    // override in bytes, read per call)
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    double budget = 0.8 * (double)free_b;
    if (const char* e = getenv("LSQ_BSOLVE_BUDGET")) budget = atof(e);
    const int64_t need = bs_need_bytes(npad, kpad);
    if ((double)need > budget) {
        int64_t kfit = kpad;
        while (kfit > 0 && (double)bs_need_bytes(npad, kfit) > budget) kfit -= BS_TB;
        kfit = std::min<int64_t>(kfit, LSQ_BORDER_MAX);
        throw Refused(std::string(who) + "a border of " + std::to_string(k) + " columns beside " + std::to_string(n) +
                      " grid columns needs " + std::to_string(need >> 20) + " MiB for Z and the border blocks, more than " +
                      std::to_string((int64_t)(budget / 1048576.0)) + " MiB (0.8 of the free device memory beside the "
                      "solver's buffers); the largest k that fits is " + std::to_string(kfit));
    }
    const auto us = [](auto a, auto c) { return (double)std::chrono::duration_cast<std::chrono::microseconds>(c - a).count(); };
    DBuf<double> Z(npad * kpad), Sm(kpad * kpad), Tm(kpad * kpad), Ri(kpad * kpad);
    DBuf<double> sk(kpad), rss(kpad), piv(kpad), asym(kpad), vss(npad), ccon(k * k), yd(std::max<int64_t>(npts, 1));
    DBuf<int64_t> dcp(k + 1);
    DBuf<int32_t> drows(std::max<int64_t>(nnzb, 1));
    DBuf<double> dvals(std::max<int64_t>(nnzb, 1));
    dcp.upload(h_cp, k + 1, st);
    drows.upload(h_rows, nnzb, st);
    dvals.upload(h_vals, nnzb, st);
    ccon.upload(h_ccon, k * k, st);
    Z.zero(st);
    Sm.zero(st);
    Tm.zero(st);
    if (S.rhs.n < std::max<int64_t>(m, 1)) S.rhs.alloc(std::max<int64_t>(m, 1));
    S.rhs.zero(st);
    HIP_CHECK(hipStreamSynchronize(st));

    // ---- steps 1, 2: one set-up (cg_available above; the multigrid levels with the first column), k solves
    lsq_opts oo = o;
    oo.method = 1;
    oo.use_x0 = 0;
    oo.b_rows = npts;
    int batch = o.batch > 0 ? o.batch : (precond == 4 ? 4 : 16);
    batch = (batch + CG_XK - 1) / CG_XK * CG_XK;
    int64_t it_total = 0, it_max = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int64_t j = 0; j < k; ++j) {
        const int64_t e0 = h_cp[j], e1 = h_cp[j + 1];
        if (npts) HIP_CHECK(hipMemsetAsync(S.rhs.p, 0, sizeof(double) * (size_t)npts, st));
        if (e1 > e0)
            hipLaunchKernelGGL(k_bs_scatter, dim3(grid_for(e1 - e0)), dim3(BLOCK), 0, st, e0, e1, drows.p, dvals.p, S.rhs.p);
        // C[:, j] = BᵗW²b_j, stored as row j (C is symmetric; its upper triangle is used)
        hipLaunchKernelGGL(k_bs_gather, dim3((unsigned)k), dim3(WAVE), 0, st, dcp.p, drows.p, dvals.p, S.rs.p, S.rhs.p,
                           Sm.p + j * kpad);
        KERNEL_CHECK();
        SetupTrace tr;
        cg_init_dev(S, S.rhs.p, nullptr, oo, precond, false, j == 0, tr);   // synchronises
        if (oo.use_graph) cg_graph_prepare(S, batch, precond);
        CgState h{};
        HIP_CHECK(hipMemcpyAsync(&h, S.cst.p, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        while (!h.stop) {
            cg_run_batch(S, batch, oo.use_graph != 0, precond);
            HIP_CHECK(hipMemcpyAsync(&h, S.cst.p, sizeof(h), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
        }
        S.cg_ready = false;
        // a column without a kept row stops at the start with z_j = 0 (istop 0, no iteration)
        if (!(h.istop == 1 || h.istop == 2 || (h.istop == 0 && h.itn == 0))) {
            S.err = std::string(who) + "the solve of border column " + std::to_string(j) + " ended with istop " +
                    std::to_string(h.istop) + " after " + std::to_string((long long)h.itn) + " iterations (maxit " +
                    std::to_string((long long)h.maxit) + "); no output was written";
            return -1;
        }
        hipLaunchKernelGGL(k_cg_xfix, dim3(grid_for(S.n_full)), dim3(BLOCK), 0, st, S.cst.p, S.n_full, cg_pbufs(S), S.cg_x.p);
        hipLaunchKernelGGL(k_cg_gather, dim3(grid_for(n)), dim3(BLOCK), 0, st, n, S.keep.p, S.cg_x.p, Z.p + j * npad);
        KERNEL_CHECK();
        it_total += h.itn;
        it_max = std::max<int64_t>(it_max, h.itn);
        if (j == 0 && h.anorm > 0.0) oo.anorm0 = std::max(o.anorm0, h.anorm);   // ‖A‖: the same operator for every column
    }
    HIP_CHECK(hipStreamSynchronize(st));
    const auto t1 = std::chrono::steady_clock::now();
    // ---- step 3: T[:, j] = Bᵗ(W² A_d z_j), stored as row j
    for (int64_t j = 0; j < k; ++j) {
        csr_spmv_rows(S, 0, npts, Z.p + j * npad, yd.p);
        hipLaunchKernelGGL(k_bs_gather, dim3((unsigned)k), dim3(WAVE), 0, st, dcp.p, drows.p, dvals.p, S.rs.p, yd.p,
                           Tm.p + j * kpad);
    }
    KERNEL_CHECK();
    HIP_CHECK(hipStreamSynchronize(st));
    const auto t2 = std::chrono::steady_clock::now();
    // ---- step 4: S̃ = s_k (C − ½(T + Tᵀ)) s_k = R̃ᵀR̃, R̃⁻¹
    hipLaunchKernelGGL(k_bs_sk, dim3(grid_for(kpad)), dim3(BLOCK), 0, st, k, kpad, Sm.p, ccon.p, sk.p);
    hipLaunchKernelGGL(k_bs_schur, dim3((unsigned)kpad), dim3(BLOCK), 0, st, k, kpad, ccon.p, Tm.p, sk.p, Sm.p, asym.p);
    KERNEL_CHECK();
    DBuf<int> err(1);
    err.zero(st);
    dense_spd_factor(Sm.p, Ri.p, kpad, err.p, st);
    int h_err = 0;
    HIP_CHECK(hipMemcpyAsync(&h_err, err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (h_err)
        throw std::invalid_argument(std::string(who) + "the border block (the Schur complement of the " + std::to_string(k) +
                                    " border columns) is not positive definite: a border column without a kept data "
                                    "row or a weighted constraint row, a c_con that is not the constraint rows' share, "
                                    "or solves too inexact for it");
    hipLaunchKernelGGL(k_bs_ri, dim3((unsigned)kpad), dim3(WAVE), 0, st, kpad, Sm.p, sk.p, Ri.p, rss.p, piv.p);
    KERNEL_CHECK();
    HIP_CHECK(hipStreamSynchronize(st));
    const auto t3 = std::chrono::steady_clock::now();
    // ---- step 5: var_add = row sums of squares of Z·(s_k R̃⁻¹)
    hipEvent_t ev0, ev1;
    HIP_CHECK(hipEventCreate(&ev0));
    HIP_CHECK(hipEventCreate(&ev1));
    HIP_CHECK(hipEventRecord(ev0, st));
    hipLaunchKernelGGL(k_bs_vss, dim3((unsigned)(npad / BS_TB)), dim3(BLOCK), 0, st, Z.p, npad, kpad, Ri.p, vss.p);
    HIP_CHECK(hipEventRecord(ev1, st));
    KERNEL_CHECK();
    HIP_CHECK(hipStreamSynchronize(st));
    float ms5 = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms5, ev0, ev1));
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    const auto t4 = std::chrono::steady_clock::now();
    // ---- step 6: op·Z in chunks of op rows, then the same quadratic form
    std::vector<double> op_add((size_t)std::max<int64_t>(nops, 0));
    if (nops > 0) {
        const int64_t nnzo = h_rp[nops];
        const int64_t chunk = std::min<int64_t>((nops + BS_TB - 1) / BS_TB * BS_TB,
                                                std::max<int64_t>(BS_TB, ((int64_t)1 << 28) / (kpad * 8) / BS_TB * BS_TB));
        DBuf<int64_t> drp(nops + 1);
        DBuf<int32_t> dci(std::max<int64_t>(nnzo, 1));
        DBuf<double> dv(std::max<int64_t>(nnzo, 1)), XZ(chunk * kpad), oss(chunk);
        drp.upload(h_rp, nops + 1, st);
        dci.upload(h_ci, nnzo, st);
        dv.upload(h_v, nnzo, st);
        for (int64_t i0 = 0; i0 < nops; i0 += chunk) {
            const int64_t cnt = std::min(chunk, nops - i0);
            XZ.zero(st);
            hipLaunchKernelGGL(k_bs_opz, dim3(grid_for(cnt, 4)), dim3(BLOCK), 0, st, i0, cnt, drp.p, dci.p, dv.p, Z.p, npad,
                               kpad, chunk, XZ.p);
            hipLaunchKernelGGL(k_bs_vss, dim3((unsigned)((cnt + BS_TB - 1) / BS_TB)), dim3(BLOCK), 0, st, XZ.p, chunk, kpad,
                               Ri.p, oss.p);
            KERNEL_CHECK();
            oss.download(op_add.data() + i0, cnt, st);
            HIP_CHECK(hipStreamSynchronize(st));
        }
    }
    const auto t5 = std::chrono::steady_clock::now();
    std::vector<double> h_piv(k), h_asym(k);
    piv.download(h_piv.data(), k, st);
    asym.download(h_asym.data(), k, st);
    vss.download(h_var_add, n, st);
    rss.download(h_var_border, k, st);
    HIP_CHECK(hipStreamSynchronize(st));
    for (int64_t i = 0; i < nops; ++i) h_op_add[i] = op_add[i];
    if (info) {
        info[0] = (double)kpad;
        info[1] = (double)need;
        info[2] = (double)it_total;
        info[3] = (double)it_max;
        info[4] = us(t0, t1);
        info[5] = us(t1, t2);
        info[6] = us(t2, t3);
        info[7] = us(t3, t4);
        info[8] = us(t4, t5);
        info[9] = *std::max_element(h_asym.begin(), h_asym.end());
        info[10] = *std::min_element(h_piv.begin(), h_piv.end());
        info[11] = (double)ms5 * 1e3;
    }
    return 0;
}
