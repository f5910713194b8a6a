// rde.hip — order statistics of scaled residuals for smooth_fit's outlier editing (SURVEY.md §8(f)
// row 1; LSsurf/RDE.py:10-18, LSsurf/calc_sigma_extra.py:13-44).
//
// calc_sigma_extra searches σ_x with RDE(r / sqrt(σ_x² + σ²)) = 1, where RDE is half the 16–84
// percentile spread — a full sort per evaluation (25–30 evaluations per outer iteration, 2–8 M
// points).  Here r and σ stay on the device; an evaluation scales, radix-sorts and returns the
// requested order statistics, and the host does numpy's interpolation and scipy's bounded Brent
// search unchanged.  The scaling is evaluated exactly as numpy does (s·s + σ·σ, correctly
// rounded sqrt and divide, compiled with -ffp-contract=off), so the sorted values — and every
// editing decision — are bit-identical to the host path.
//
// Segmented select (binned sigma_extra, calc_sigma_extra_on_grid): many overlapping (bin × group)
// segments of one point set, each with its own trial σ_x per evaluation.  RDE needs four order
// statistics, not a sorted array, so lsq_rde_select finds them by an MSB-first radix select over
// order-preserving 64-bit keys of x (8 digits of 8 bits, integer histograms only — exact and
// independent of the order of the atomics).  Segments of up to SMALL_MAX points run one workgroup
// each with their keys resident in LDS (all passes inside one kernel); larger ones run
// multi-workgroup histogram passes whose bucket decisions are taken on the device, so an
// evaluation is a fixed launch sequence and one device-to-host copy.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lsqsurf.h"
#include "common.hpp"

struct lsq_rde {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t n = 0;
    lsq::DBuf<double> r, sig, x, xs;
    lsq::DBuf<unsigned char> tmp;
    size_t tmp_bytes = 0;
    std::string err;
    // segmented select (lsq_rde_create_segments)
    bool segmented = false;
    int64_t n_seg = 0, total = 0, n_large = 0;
    std::vector<int64_t> h_ptr;             // seg_ptr on the host (classing the active list)
    lsq::DBuf<double> rs, ss;               // segment-contiguous copies of r and σ
    lsq::DBuf<unsigned long long> key;      // keys of the large segments' current evaluation
    lsq::DBuf<int64_t> d_ptr, d_rank;
    lsq::DBuf<unsigned char> d_act;         // active list of one evaluation (SelAct)
    lsq::DBuf<unsigned char> d_state;       // per active large segment (SelState)
    lsq::DBuf<double> d_out;
};

namespace {

// ---- segmented radix select ---------------------------------------------------------------
constexpr int SEL_BITS = 8, SEL_BUCKETS = 1 << SEL_BITS, SEL_PASSES = 64 / SEL_BITS;
// One workgroup may hold 160 KiB of LDS on gfx950: 16384 keys = 128 KiB plus 2 KiB of histograms
// leaves the largest class one workgroup per CU; the smaller classes keep more of them resident.
constexpr int SMALL_MAX = 16384;
constexpr int SMALL_CAPS[3] = {2048, 8192, SMALL_MAX};
constexpr int LARGE_ITEMS = 16;        // keys per thread and pass the large path's grid is sized for
constexpr int LARGE_CHUNKS_MAX = 256;  // workgroups per segment at most

struct SelAct {      // one active segment of an evaluation
    int32_t seg, slot;
    double s;
};
struct SelState {    // select state of one active large segment; pair 0 = (j_lo, j_lo+1), 1 = (j_hi, j_hi+1)
    unsigned long long prefix[2], next[2];
    int64_t k[2];
    uint32_t eq[2];
    uint32_t hist[2][SEL_BUCKETS];
};

// Order-preserving key of a double: negative values flip every bit, the others the sign bit, so
// unsigned key order = numeric order (−0 sorts just below +0; NaN, which np.sort puts last, gets
// the largest key).
__device__ __forceinline__ unsigned long long sel_key(double x) {
    if (x != x) return ~0ull;
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double sel_value(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}
// x exactly as k_scaled forms it (raw: r itself)
__device__ __forceinline__ unsigned long long sel_key_of(double r, double sig, double s2, int raw) {
    if (raw) return sel_key(r);
    const double q = sig * sig;
    return sel_key(r / sqrt(s2 + q));
}
__device__ __forceinline__ unsigned long long sel_mask(int pass) {   // digits decided before `pass`
    return pass == 0 ? 0ull : ~0ull << (64 - SEL_BITS * pass);
}

// One full wave: the bucket of `h` (SEL_BUCKETS counts) that holds 0-based rank k, the count below
// that bucket and the bucket's own count.  Every lane returns the same values.
__device__ __forceinline__ void sel_pick(const uint32_t* h, int64_t k, int& bucket, uint32_t& below, uint32_t& cnt) {
    const int lane = threadIdx.x & 63;
    uint32_t c[4], t = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[i] = h[4 * lane + i];
        t += c[i];
    }
    uint32_t inc = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
    }
    const unsigned long long m = __ballot((int64_t)inc > k);
    const int first = m ? __ffsll((long long)m) - 1 : 63;
    int b = 4 * lane;
    uint32_t lo = inc - t, n = c[0];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if ((int64_t)(lo + n) <= k) {
            lo += n;
            n = c[i + 1];
            ++b;
        }
    bucket = __shfl(b, first, 64);
    below = __shfl(lo, first, 64);
    cnt = __shfl(n, first, 64);
}

__global__ __launch_bounds__(lsq::BLOCK) void k_seg_gather(int64_t total, const int32_t* __restrict__ idx,
                                                           const double* __restrict__ r,
                                                           const double* __restrict__ sig, double* __restrict__ rs,
                                                           double* __restrict__ ss) {
    for (int64_t i = (int64_t)blockIdx.x * lsq::BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * lsq::BLOCK) {
        const int32_t p = idx[i];
        rs[i] = r[p];
        ss[i] = sig[p];
    }
}

// Small segments: one workgroup per active segment, keys in LDS, every pass in this kernel.
template <int CAP>
__global__ __launch_bounds__(lsq::BLOCK) void k_select_small(const SelAct* __restrict__ act,
                                                             const int64_t* __restrict__ seg_ptr,
                                                             const int64_t* __restrict__ seg_rank,
                                                             const double* __restrict__ rs,
                                                             const double* __restrict__ ss, int raw,
                                                             double* __restrict__ out) {
    __shared__ unsigned long long keys[CAP];
    __shared__ uint32_t hist[2][SEL_BUCKETS];
    __shared__ unsigned long long prefix[2], next[2];
    __shared__ int64_t kk[2];
    __shared__ uint32_t eq[2];
    const SelAct a = act[blockIdx.x];
    const int64_t p0 = seg_ptr[a.seg];
    const int len = (int)(seg_ptr[a.seg + 1] - p0);   // ≤ CAP: the host classes the active list
    const int tid = threadIdx.x, wave = tid >> 6;
    const double s2 = a.s * a.s;
    for (int i = tid; i < len; i += lsq::BLOCK) keys[i] = sel_key_of(rs[p0 + i], ss[p0 + i], s2, raw);
    if (tid < 2) {
        prefix[tid] = 0;
        next[tid] = ~0ull;
        kk[tid] = seg_rank[4 * (int64_t)a.seg + 2 * tid];
    }
    for (int pass = 0; pass < SEL_PASSES; ++pass) {
        hist[0][tid] = 0;
        hist[1][tid] = 0;
        __syncthreads();
        const unsigned long long m = sel_mask(pass), f0 = prefix[0], f1 = prefix[1];
        const int shift = 64 - SEL_BITS * (pass + 1);
        for (int i = tid; i < len; i += lsq::BLOCK) {
            const unsigned long long key = keys[i];
            const int d = (int)(key >> shift) & (SEL_BUCKETS - 1);
            if (((key ^ f0) & m) == 0) atomicAdd(&hist[0][d], 1u);
            if (((key ^ f1) & m) == 0) atomicAdd(&hist[1][d], 1u);
        }
        __syncthreads();
        if (wave < 2) {
            int b;
            uint32_t below, cnt;
            sel_pick(hist[wave], kk[wave], b, below, cnt);
            if ((tid & 63) == 0) {
                prefix[wave] |= (unsigned long long)b << shift;
                kk[wave] -= below;
                eq[wave] = cnt;
            }
        }
        __syncthreads();
    }
    // v_{j+1} = v_j when another element equals it, else the smallest element above v_j
    const unsigned long long v0 = prefix[0], v1 = prefix[1];
    unsigned long long n0 = ~0ull, n1 = ~0ull;
    for (int i = tid; i < len; i += lsq::BLOCK) {
        const unsigned long long key = keys[i];
        if (key > v0 && key < n0) n0 = key;
        if (key > v1 && key < n1) n1 = key;
    }
    if (n0 != ~0ull) atomicMin(&next[0], n0);
    if (n1 != ~0ull) atomicMin(&next[1], n1);
    __syncthreads();
    if (tid < 2) {
        double* o = out + 4 * (int64_t)a.slot + 2 * tid;
        o[0] = sel_value(prefix[tid]);
        o[1] = sel_value((int64_t)eq[tid] > kk[tid] + 1 ? prefix[tid] : next[tid]);
    }
}

// Large segments: grid (active large segment, chunk of it).
__global__ void k_large_init(const SelAct* __restrict__ act, const int64_t* __restrict__ seg_rank,
                             SelState* __restrict__ st) {
    SelState& s = st[blockIdx.x];
    const int tid = threadIdx.x;
    s.hist[0][tid] = 0;
    s.hist[1][tid] = 0;
    if (tid < 2) {
        s.prefix[tid] = 0;
        s.next[tid] = ~0ull;
        s.k[tid] = seg_rank[4 * (int64_t)act[blockIdx.x].seg + 2 * tid];
        s.eq[tid] = 0;
    }
}

__global__ __launch_bounds__(lsq::BLOCK) void k_large_keys(const SelAct* __restrict__ act,
                                                           const int64_t* __restrict__ seg_ptr,
                                                           const double* __restrict__ rs,
                                                           const double* __restrict__ ss, int raw,
                                                           unsigned long long* __restrict__ key) {
    const SelAct a = act[blockIdx.x];
    const int64_t p0 = seg_ptr[a.seg], p1 = seg_ptr[a.seg + 1];
    const double s2 = a.s * a.s;
    for (int64_t i = p0 + (int64_t)blockIdx.y * lsq::BLOCK + threadIdx.x; i < p1; i += (int64_t)gridDim.y * lsq::BLOCK)
        key[i] = sel_key_of(rs[i], ss[i], s2, raw);
}

__global__ __launch_bounds__(lsq::BLOCK) void k_large_hist(const SelAct* __restrict__ act,
                                                           const int64_t* __restrict__ seg_ptr,
                                                           const unsigned long long* __restrict__ key, int pass,
                                                           SelState* __restrict__ st) {
    __shared__ uint32_t hist[2][SEL_BUCKETS];
    const int seg = act[blockIdx.x].seg, tid = threadIdx.x;
    const int64_t p0 = seg_ptr[seg], p1 = seg_ptr[seg + 1];
    if (p0 + (int64_t)blockIdx.y * lsq::BLOCK >= p1) return;   // whole workgroup: nothing of this segment
    SelState& s = st[blockIdx.x];
    hist[0][tid] = 0;
    hist[1][tid] = 0;
    __syncthreads();
    const unsigned long long m = sel_mask(pass), f0 = s.prefix[0], f1 = s.prefix[1];
    const int shift = 64 - SEL_BITS * (pass + 1);
    for (int64_t i = p0 + (int64_t)blockIdx.y * lsq::BLOCK + tid; i < p1; i += (int64_t)gridDim.y * lsq::BLOCK) {
        const unsigned long long k = key[i];
        const int d = (int)(k >> shift) & (SEL_BUCKETS - 1);
        if (((k ^ f0) & m) == 0) atomicAdd(&hist[0][d], 1u);
        if (((k ^ f1) & m) == 0) atomicAdd(&hist[1][d], 1u);
    }
    __syncthreads();
    if (hist[0][tid]) atomicAdd(&s.hist[0][tid], hist[0][tid]);
    if (hist[1][tid]) atomicAdd(&s.hist[1][tid], hist[1][tid]);
}

// The bucket decision of one pass, on the device: 128 threads, one wave per rank pair.
__global__ void k_large_decide(int pass, SelState* __restrict__ st) {
    SelState& s = st[blockIdx.x];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int b;
    uint32_t below, cnt;
    sel_pick(s.hist[wave], s.k[wave], b, below, cnt);
    __syncthreads();
    for (int i = lane; i < SEL_BUCKETS; i += 64) s.hist[wave][i] = 0;
    if (lane == 0) {
        s.prefix[wave] |= (unsigned long long)b << (64 - SEL_BITS * (pass + 1));
        s.k[wave] -= below;
        s.eq[wave] = cnt;
    }
}

__global__ __launch_bounds__(lsq::BLOCK) void k_large_next(const SelAct* __restrict__ act,
                                                           const int64_t* __restrict__ seg_ptr,
                                                           const unsigned long long* __restrict__ key,
                                                           SelState* __restrict__ st) {
    __shared__ unsigned long long next[2];
    const int seg = act[blockIdx.x].seg, tid = threadIdx.x;
    const int64_t p0 = seg_ptr[seg], p1 = seg_ptr[seg + 1];
    if (p0 + (int64_t)blockIdx.y * lsq::BLOCK >= p1) return;
    SelState& s = st[blockIdx.x];
    if (tid < 2) next[tid] = ~0ull;
    __syncthreads();
    const unsigned long long v0 = s.prefix[0], v1 = s.prefix[1];
    unsigned long long n0 = ~0ull, n1 = ~0ull;
    for (int64_t i = p0 + (int64_t)blockIdx.y * lsq::BLOCK + tid; i < p1; i += (int64_t)gridDim.y * lsq::BLOCK) {
        const unsigned long long k = key[i];
        if (k > v0 && k < n0) n0 = k;
        if (k > v1 && k < n1) n1 = k;
    }
    if (n0 != ~0ull) atomicMin(&next[0], n0);
    if (n1 != ~0ull) atomicMin(&next[1], n1);
    __syncthreads();
    if (tid < 2 && next[tid] != ~0ull) atomicMin(&s.next[tid], next[tid]);
}

__global__ void k_large_out(int64_t n_large, const SelAct* __restrict__ act, const SelState* __restrict__ st,
                            double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * n_large) return;
    const SelState& s = st[t >> 1];
    const int p = (int)(t & 1);
    double* o = out + 4 * (int64_t)act[t >> 1].slot + 2 * p;
    o[0] = sel_value(s.prefix[p]);
    o[1] = sel_value((int64_t)s.eq[p] > s.k[p] + 1 ? s.prefix[p] : s.next[p]);
}

std::string g_create_err;   // why the last lsq_rde_create_segments returned NULL

__global__ __launch_bounds__(lsq::BLOCK) void k_scaled(int64_t n, const double* __restrict__ r,
                                                       const double* __restrict__ sig, double s,
                                                       double* __restrict__ x) {
    const double s2 = s * s;
    for (int64_t i = (int64_t)blockIdx.x * lsq::BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * lsq::BLOCK) {
        const double q = sig[i] * sig[i];
        x[i] = r[i] / sqrt(s2 + q);
    }
}

__global__ void k_pick(int64_t n, const double* __restrict__ xs, int64_t m, const int64_t* __restrict__ idx,
                       double* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < m) out[k] = xs[idx[k]];
}

}  // namespace

extern "C" {

lsq_rde* lsq_rde_create(int32_t device, int64_t n, const double* r, const double* sigma) {
    if (n < 1 || !r || !sigma) return nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return nullptr;
    auto* c = new lsq_rde();
    try {
        HIP_CHECK(hipSetDevice(device));
        c->device = device;
        HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->n = n;
        c->r.alloc(n);
        c->sig.alloc(n);
        c->x.alloc(n);
        c->xs.alloc(n);
        c->r.upload(r, n, c->stream);
        c->sig.upload(sigma, n, c->stream);
        HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(nullptr, c->tmp_bytes, c->x.p, c->xs.p, (int)n, 0, 64,
                                                    c->stream));
        c->tmp.alloc((int64_t)c->tmp_bytes + 1);
        HIP_CHECK(hipStreamSynchronize(c->stream));
    } catch (const std::exception&) {
        lsq_rde_destroy(c);
        return nullptr;
    }
    return c;
}

int lsq_rde_order_stats(lsq_rde* c, double sigma_extra, int64_t n_idx, const int64_t* idx, double* out) {
    if (!c) return -1;
    try {
        if (c->segmented) throw std::invalid_argument("lsq_rde_order_stats: a segmented context (use lsq_rde_select)");
        if (n_idx < 0 || (n_idx && (!idx || !out))) throw std::invalid_argument("lsq_rde_order_stats: bad args");
        for (int64_t k = 0; k < n_idx; ++k)
            if (idx[k] < 0 || idx[k] >= c->n) throw std::invalid_argument("lsq_rde_order_stats: index out of range");
        HIP_CHECK(hipSetDevice(c->device));
        hipLaunchKernelGGL(k_scaled, dim3(lsq::grid_for(c->n)), dim3(lsq::BLOCK), 0, c->stream, c->n, c->r.p,
                           c->sig.p, sigma_extra, c->x.p);
        KERNEL_CHECK();
        HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(c->tmp.p, c->tmp_bytes, c->x.p, c->xs.p, (int)c->n, 0, 64,
                                                    c->stream));
        if (n_idx) {
            lsq::DBuf<int64_t> di(n_idx);
            lsq::DBuf<double> dout(n_idx);
            di.upload(idx, n_idx, c->stream);
            hipLaunchKernelGGL(k_pick, dim3((unsigned)((n_idx + 63) / 64)), dim3(64), 0, c->stream, c->n, c->xs.p, n_idx,
                               di.p, dout.p);
            KERNEL_CHECK();
            dout.download(out, n_idx, c->stream);
            HIP_CHECK(hipStreamSynchronize(c->stream));
        }
        return 0;
    } catch (const std::invalid_argument& e) {
        c->err = e.what();
        return -2;
    } catch (const std::exception& e) {
        c->err = e.what();
        return -3;
    }
}

int64_t lsq_rde_small_max(void) { return SMALL_MAX; }

lsq_rde* lsq_rde_create_segments(int32_t device, int64_t n, const double* r, const double* sigma, int64_t n_seg,
                                 const int64_t* seg_ptr, const int32_t* seg_idx, const int64_t* seg_rank,
                                 int* status) {
    static_assert(lsq::BLOCK == SEL_BUCKETS, "one histogram bucket per thread");
    int st = 0;
    lsq_rde* c = nullptr;
    g_create_err.clear();
    try {
        if (n < 1 || n_seg < 1 || !r || !sigma || !seg_ptr || !seg_idx || !seg_rank)
            throw std::invalid_argument("lsq_rde_create_segments: bad args");
        if (n_seg >= (int64_t)1 << 31) throw std::invalid_argument("lsq_rde_create_segments: too many segments");
        if (seg_ptr[0] != 0) throw std::invalid_argument("lsq_rde_create_segments: seg_ptr[0] must be 0");
        int64_t n_large = 0;
        for (int64_t k = 0; k < n_seg; ++k) {
            const int64_t len = seg_ptr[k + 1] - seg_ptr[k];
            if (len < 0) throw std::invalid_argument("lsq_rde_create_segments: seg_ptr is not monotone");
            const int64_t* q = seg_rank + 4 * k;
            for (int i = 0; i < 4; ++i)
                if (q[i] < 0 || q[i] >= len)
                    throw std::invalid_argument("lsq_rde_create_segments: rank outside its segment");
            if (q[1] != q[0] + 1 || q[3] != q[2] + 1)
                throw std::invalid_argument("lsq_rde_create_segments: ranks must be (j_lo, j_lo+1, j_hi, j_hi+1)");
            n_large += len > SMALL_MAX;
        }
        const int64_t total = seg_ptr[n_seg];
        if (total >= (int64_t)1 << 31) throw lsq::Refused("lsq_rde_create_segments: 2^31 or more segment entries");
        for (int64_t i = 0; i < total; ++i)
            if (seg_idx[i] < 0 || seg_idx[i] >= n)
                throw std::invalid_argument("lsq_rde_create_segments: point index out of range");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
            throw lsq::HipError("lsq_rde_create_segments: no such device");
        HIP_CHECK(hipSetDevice(device));
        // r, σ and the index list only live through the gather; the copies, the keys and the
        // per-segment tables stay
        const double need = 24.0 * total + 16.0 * n + 4.0 * total + 80.0 * n_seg + (double)sizeof(SelState) * n_large;
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        if (need > 0.8 * (double)free_b)
            throw lsq::Refused("lsq_rde_create_segments: " + std::to_string((int64_t)need) +
                               " bytes do not fit the device's free memory");
        c = new lsq_rde();
        c->device = device;
        c->segmented = true;
        HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->n = n;
        c->n_seg = n_seg;
        c->total = total;
        c->n_large = n_large;
        c->h_ptr.assign(seg_ptr, seg_ptr + n_seg + 1);
        c->rs.alloc(total);
        c->ss.alloc(total);
        c->key.alloc(n_large ? total : 0);
        c->d_ptr.alloc(n_seg + 1);
        c->d_rank.alloc(4 * n_seg);
        c->d_ptr.upload(seg_ptr, n_seg + 1, c->stream);
        c->d_rank.upload(seg_rank, 4 * n_seg, c->stream);
        {
            lsq::DBuf<double> dr(n), ds(n);
            lsq::DBuf<int32_t> di(total);
            dr.upload(r, n, c->stream);
            ds.upload(sigma, n, c->stream);
            di.upload(seg_idx, total, c->stream);
            hipLaunchKernelGGL(k_seg_gather, dim3(lsq::grid_for(total)), dim3(lsq::BLOCK), 0, c->stream, total, di.p,
                               dr.p, ds.p, c->rs.p, c->ss.p);
            KERNEL_CHECK();
            HIP_CHECK(hipStreamSynchronize(c->stream));
        }
    } catch (const lsq::Refused& e) {
        g_create_err = e.what();
        st = -5;
    } catch (const std::invalid_argument& e) {
        g_create_err = e.what();
        st = -2;
    } catch (const std::exception& e) {
        g_create_err = e.what();
        st = -3;
    }
    if (st != 0 && c) {
        lsq_rde_destroy(c);
        c = nullptr;
    }
    if (status) *status = st;
    return c;
}

int lsq_rde_select(lsq_rde* c, int64_t n_act, const int32_t* seg, const double* s, int32_t raw, double* out) {
    if (!c) return -1;
    try {
        if (!c->segmented) throw std::invalid_argument("lsq_rde_select: not a segmented context (use lsq_rde_order_stats)");
        if (n_act < 0 || n_act >= (int64_t)1 << 31 || (n_act && (!seg || !s || !out)))
            throw std::invalid_argument("lsq_rde_select: bad args");
        if (n_act == 0) return 0;
        // class the active list: the three LDS capacities, then the multi-workgroup path
        std::vector<SelAct> act((size_t)n_act);
        int64_t cnt[4] = {0, 0, 0, 0}, off[5] = {0, 0, 0, 0, 0};
        std::vector<unsigned char> cls((size_t)n_act);
        int64_t max_large = 0;
        std::vector<unsigned char> seen((size_t)c->n_seg, 0);
        for (int64_t a = 0; a < n_act; ++a) {
            if (seg[a] < 0 || seg[a] >= c->n_seg) throw std::invalid_argument("lsq_rde_select: segment id out of range");
            if (seen[seg[a]]++) throw std::invalid_argument("lsq_rde_select: a segment is listed twice");
            const int64_t len = c->h_ptr[seg[a] + 1] - c->h_ptr[seg[a]];
            int k = 0;
            while (k < 3 && len > SMALL_CAPS[k]) ++k;
            if (k == 3) max_large = std::max(max_large, len);
            cls[a] = (unsigned char)k;
            ++cnt[k];
        }
        for (int k = 0; k < 4; ++k) off[k + 1] = off[k] + cnt[k];
        int64_t pos[4] = {off[0], off[1], off[2], off[3]};
        for (int64_t a = 0; a < n_act; ++a) act[pos[cls[a]]++] = SelAct{seg[a], (int32_t)a, s[a]};

        HIP_CHECK(hipSetDevice(c->device));
        if (c->d_act.n < n_act * (int64_t)sizeof(SelAct)) c->d_act.alloc(n_act * (int64_t)sizeof(SelAct));
        if (c->d_out.n < 4 * n_act) c->d_out.alloc(4 * n_act);
        if (c->d_state.n < cnt[3] * (int64_t)sizeof(SelState)) c->d_state.alloc(cnt[3] * (int64_t)sizeof(SelState));
        HIP_CHECK(hipMemcpyAsync(c->d_act.p, act.data(), sizeof(SelAct) * (size_t)n_act, hipMemcpyHostToDevice,
                                 c->stream));
        const SelAct* dact = reinterpret_cast<const SelAct*>(c->d_act.p);
        const int iraw = raw ? 1 : 0;
        if (cnt[0]) {
            hipLaunchKernelGGL(k_select_small<SMALL_CAPS[0]>, dim3((unsigned)cnt[0]), dim3(lsq::BLOCK), 0, c->stream,
                               dact + off[0], c->d_ptr.p, c->d_rank.p, c->rs.p, c->ss.p, iraw, c->d_out.p);
            KERNEL_CHECK();
        }
        if (cnt[1]) {
            hipLaunchKernelGGL(k_select_small<SMALL_CAPS[1]>, dim3((unsigned)cnt[1]), dim3(lsq::BLOCK), 0, c->stream,
                               dact + off[1], c->d_ptr.p, c->d_rank.p, c->rs.p, c->ss.p, iraw, c->d_out.p);
            KERNEL_CHECK();
        }
        if (cnt[2]) {
            hipLaunchKernelGGL(k_select_small<SMALL_CAPS[2]>, dim3((unsigned)cnt[2]), dim3(lsq::BLOCK), 0, c->stream,
                               dact + off[2], c->d_ptr.p, c->d_rank.p, c->rs.p, c->ss.p, iraw, c->d_out.p);
            KERNEL_CHECK();
        }
        // the large path: grid x carries the segment (slices of 32768), grid y its chunks
        for (int64_t l0 = 0; l0 < cnt[3]; l0 += 32768) {
            const unsigned nl = (unsigned)std::min<int64_t>(32768, cnt[3] - l0);
            const SelAct* la = dact + off[3] + l0;
            SelState* st = reinterpret_cast<SelState*>(c->d_state.p) + l0;
            int64_t chunks = (max_large + (int64_t)lsq::BLOCK * LARGE_ITEMS - 1) / ((int64_t)lsq::BLOCK * LARGE_ITEMS);
            chunks = std::min<int64_t>(std::max<int64_t>(chunks, 1), LARGE_CHUNKS_MAX);
            const dim3 grid(nl, (unsigned)chunks);
            hipLaunchKernelGGL(k_large_init, dim3(nl), dim3(SEL_BUCKETS), 0, c->stream, la, c->d_rank.p, st);
            KERNEL_CHECK();
            hipLaunchKernelGGL(k_large_keys, grid, dim3(lsq::BLOCK), 0, c->stream, la, c->d_ptr.p, c->rs.p, c->ss.p,
                               iraw, c->key.p);
            KERNEL_CHECK();
            for (int pass = 0; pass < SEL_PASSES; ++pass) {
                hipLaunchKernelGGL(k_large_hist, grid, dim3(lsq::BLOCK), 0, c->stream, la, c->d_ptr.p, c->key.p, pass,
                                   st);
                KERNEL_CHECK();
                hipLaunchKernelGGL(k_large_decide, dim3(nl), dim3(128), 0, c->stream, pass, st);
                KERNEL_CHECK();
            }
            hipLaunchKernelGGL(k_large_next, grid, dim3(lsq::BLOCK), 0, c->stream, la, c->d_ptr.p, c->key.p, st);
            KERNEL_CHECK();
            hipLaunchKernelGGL(k_large_out, dim3((2 * nl + 63) / 64), dim3(64), 0, c->stream, (int64_t)nl, la, st,
                               c->d_out.p);
            KERNEL_CHECK();
        }
        c->d_out.download(out, 4 * n_act, c->stream);
        HIP_CHECK(hipStreamSynchronize(c->stream));
        return 0;
    } catch (const std::invalid_argument& e) {
        c->err = e.what();
        return -2;
    } catch (const std::exception& e) {
        c->err = e.what();
        return -3;
    }
}

const char* lsq_rde_last_error(lsq_rde* c) {
    if (c) return c->err.c_str();
    return g_create_err.empty() ? "null rde context" : g_create_err.c_str();
}

void lsq_rde_destroy(lsq_rde* c) {
    if (!c) return;
    c->rs.release();
    c->ss.release();
    c->key.release();
    c->d_ptr.release();
    c->d_rank.release();
    c->d_act.release();
    c->d_state.release();
    c->d_out.release();
    c->r.release();
    c->sig.release();
    c->x.release();
    c->xs.release();
    c->tmp.release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

}  // extern "C"
