// Measurement passes of the per-layer quantisation report (utils/report.py): HBM-bound streaming kernels, one pass over each input,
// nothing of the input's size written.
//   adalog_err_stats_f32         per channel: sum (a-b)^2, sum a^2, sum b^2, max |a-b| in fp64                      (k_stats<Acc>)
//   adalog_mean_err_f32          per channel: sum (a-b), sum (a-b)^2, max |a| in fp64 (utils/bias_correct.py)       (k_stats<MeanAcc>)
//   adalog_uniform_code_hist_f32 per channel: counts of the codes rne(x/s) + rne(z) and of the two clip sides       (k_code_hist_uniform)
//   adalog_log_code_hist_f32     counts of the AdaLog / ShiftAdaLog bins and of the masked code                      (k_code_hist_log)
// Channel convention of the uniform quantiser (fakequant.hip): channel(i) = (i / inner) % n_channels, i.e. the tensor is
// [rpc][n_channels][inner] and channel c owns rpc rows of inner contiguous elements.
//
// Reproducibility: no floating-point atomics.  err_stats and mean_err write one fp64 partial per (channel, block) to the caller's workspace and a
// second small launch adds them in a fixed order (block partials: lanes, then waves, in a fixed tree), so two runs give the same bits.
// The histograms count in 32-bit LDS counters private to a wave (several copies per wave for narrow codes: 64 lanes on 16 counters
// would serialise on the same address) and flush with 64-bit integer atomics: integer sums do not depend on the order.
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MAX_PARTS = 2048;                        // blocks per channel at most (grid-stride the rest)
constexpr int64_t MAX_N = (int64_t)1 << 40;            // keeps a block's share below 2^31 elements: the 32-bit LDS counters cannot wrap

struct Geo {
    int64_t inner, n_ch, rpc;                          // rpc: rows per channel
    int vec;                                           // rpc > 1: every row starts 16-byte aligned and holds whole float4s
};

// f(a[i], b[i]) for every element i of channel c that falls to this block (blockIdx.x of gridDim.x).  16-byte loads wherever the
// addresses allow: a channel that is one contiguous run (per-tensor, one row per channel) peels a scalar head up to the first aligned
// element and a scalar tail; rows of a multi-row channel are vectorised when all of them are aligned.  TWO = false: b is not read.
template <bool TWO, class F>
__device__ __forceinline__ void stream_channel(const float* __restrict__ a, const float* __restrict__ b, const Geo& g, int64_t c, F&& f) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    if (g.rpc == 1) {
        const float* pa = a + c * g.inner;
        const float* pb = TWO ? b + c * g.inner : pa;
        const int64_t len = g.inner;
        int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)pa & 15u)) & 15u) >> 2);
        if (head > len || (TWO && (((uintptr_t)pa ^ (uintptr_t)pb) & 15u) != 0)) head = len;    // (a and b aligned differently: scalar)
        const int64_t n4 = (len - head) >> 2, tail0 = head + 4 * n4;
        const float4* va = reinterpret_cast<const float4*>(pa + head);
        const float4* vb = reinterpret_cast<const float4*>(pb + head);
        for (int64_t i = tid; i < n4; i += nth) {
            const float4 x = va[i];
            const float4 y = TWO ? vb[i] : x;
            f(x.x, y.x); f(x.y, y.y); f(x.z, y.z); f(x.w, y.w);
        }
        const int64_t ns = head + (len - tail0);
        for (int64_t i = tid; i < ns; i += nth) {
            const int64_t j = i < head ? i : tail0 + (i - head);
            f(pa[j], pb[j]);
        }
    } else if (g.vec) {
        const int64_t i4 = g.inner >> 2, n4 = g.rpc * i4;
        const float4* va = reinterpret_cast<const float4*>(a);
        const float4* vb = reinterpret_cast<const float4*>(TWO ? b : a);
        for (int64_t i = tid; i < n4; i += nth) {
            const int64_t r = i / i4, c4 = i - r * i4;
            const int64_t o = (r * g.n_ch + c) * i4 + c4;
            const float4 x = va[o];
            const float4 y = TWO ? vb[o] : x;
            f(x.x, y.x); f(x.y, y.y); f(x.z, y.z); f(x.w, y.w);
        }
    } else {
        const int64_t m = g.rpc * g.inner;
        const float* pb = TWO ? b : a;
        for (int64_t i = tid; i < m; i += nth) {
            const int64_t r = i / g.inner, col = i - r * g.inner;
            const int64_t o = (r * g.n_ch + c) * g.inner + col;
            f(a[o], pb[o]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ error statistics
// An accumulator is N fp64 values v[] with add(x, y) for one element pair and merge(o) for another accumulator: the kernels below
// (stream or cols pass, block tree, finish) are written once over it.
struct Acc {                                           // err_stats: sum (a-b)^2, sum a^2, sum b^2, max |a-b|
    static constexpr int N = 4;
    double v[N];
    __device__ __forceinline__ void add(float x, float y) {
        const double dx = (double)x, dy = (double)y, d = dx - dy;     // fp64 from the fp32 inputs: no fp32 rounding, no fp32 overflow
        v[0] += d * d;
        v[1] += dx * dx;
        v[2] += dy * dy;
        v[3] = fmax(v[3], fabs(d));
    }
    __device__ __forceinline__ void merge(const Acc& o) { v[0] += o.v[0]; v[1] += o.v[1]; v[2] += o.v[2]; v[3] = fmax(v[3], o.v[3]); }
};

struct MeanAcc {                                       // mean_err: sum (a-b), sum (a-b)^2, max |a|
    static constexpr int N = 3;
    double v[N];
    __device__ __forceinline__ void add(float x, float y) {
        const double dx = (double)x, d = dx - (double)y;              // exact: the difference of two fp32 values fits fp64's exponent range
        v[0] += d;
        v[1] += d * d;
        v[2] = fmax(v[2], fabs(dx));
    }
    __device__ __forceinline__ void merge(const MeanAcc& o) { v[0] += o.v[0]; v[1] += o.v[1]; v[2] = fmax(v[2], o.v[2]); }
};

template <class A> __device__ __forceinline__ A zero_acc() {
    A a;
#pragma unroll
    for (int k = 0; k < A::N; ++k) a.v[k] = 0.0;
    return a;
}

// the block's accumulator in thread 0: lanes by shuffles (a fixed tree), then the waves in order
template <class A>
__device__ __forceinline__ A block_reduce(A v, A* red /* [WAVES] in LDS */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        A o;
#pragma unroll
        for (int k = 0; k < A::N; ++k) o.v[k] = __shfl_down(v.v[k], off);
        v.merge(o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < WAVES; ++w) v.merge(red[w]);
    __syncthreads();                                   // red is reused by the next channel of this block
    return v;
}

template <class A> __device__ __forceinline__ void store_acc(double* p, const A& a) {
#pragma unroll
    for (int k = 0; k < A::N; ++k) p[k] = a.v[k];
}

// part[c][blockIdx.x][N]: the share of block blockIdx.x (of gridDim.x = parts) in channel c
template <class A>
__global__ __launch_bounds__(TPB) void k_stats(const float* __restrict__ a, const float* __restrict__ b, Geo g, double* __restrict__ part) {
    __shared__ A red[WAVES];
    for (int64_t c = blockIdx.y; c < g.n_ch; c += gridDim.y) {
        A v = zero_acc<A>();
        stream_channel<true>(a, b, g, c, [&](float x, float y) { v.add(x, y); });
        v = block_reduce(v, red);
        if (threadIdx.x == 0) store_acc(part + (c * gridDim.x + blockIdx.x) * A::N, v);
    }
}

// inner = 1: x is [rows][n_ch], a thread owns a channel (coalesced along the channels) and every parts-th row of it
template <class A>
__global__ __launch_bounds__(TPB) void k_stats_cols(const float* __restrict__ a, const float* __restrict__ b, int64_t rows, int64_t n_ch,
                                                    double* __restrict__ part) {
    const int64_t ch = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= n_ch) return;
    A v = zero_acc<A>();
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) v.add(a[r * n_ch + ch], b[r * n_ch + ch]);
    store_acc(part + (ch * gridDim.y + blockIdx.y) * A::N, v);
}

// out[c][N] = the parts of channel c added in a fixed order: thread t takes parts t, t + 256, ... in order, then the block's tree
template <class A>
__global__ __launch_bounds__(TPB) void k_stats_finish(const double* __restrict__ part, int64_t n_ch, int parts, double* __restrict__ out) {
    __shared__ A red[WAVES];
    for (int64_t c = blockIdx.x; c < n_ch; c += gridDim.x) {
        A v = zero_acc<A>();
        for (int p = threadIdx.x; p < parts; p += TPB) {
            const double* q = part + (c * parts + p) * A::N;
            A o;
#pragma unroll
            for (int k = 0; k < A::N; ++k) o.v[k] = q[k];
            v.merge(o);
        }
        v = block_reduce(v, red);
        if (threadIdx.x == 0) store_acc(out + c * A::N, v);
    }
}

// ------------------------------------------------------------------------------------------------ code histograms
// copies of a wave's counters (lane l counts in copy l % COPIES): as many as keep a wave's counters within ~288 words
template <int NB> constexpr int copies_for() { return NB <= 18 ? 16 : NB <= 34 ? 8 : NB <= 66 ? 4 : NB <= 130 ? 2 : 1; }

template <int NB>
struct Counters {
    static constexpr int COPIES = copies_for<NB>();
    static constexpr int WORDS = WAVES * COPIES * NB;
    __device__ static __forceinline__ void clear(unsigned int* cnt) {
        for (int i = threadIdx.x; i < WORDS; i += TPB) cnt[i] = 0u;
        __syncthreads();
    }
    __device__ static __forceinline__ unsigned int* mine(unsigned int* cnt) {
        return cnt + ((threadIdx.x >> 6) * COPIES + (threadIdx.x & (COPIES - 1))) * NB;
    }
    // out[bin] += the block's count of bin (64-bit integer atomics: the result does not depend on the order)
    __device__ static __forceinline__ void flush(unsigned int* cnt, unsigned long long* out) {
        __syncthreads();
        for (int bin = threadIdx.x; bin < NB; bin += TPB) {
            unsigned long long t = 0;
            for (int k = 0; k < WAVES * COPIES; ++k) t += cnt[k * NB + bin];
            if (t) atomicAdd(out + bin, t);
        }
        __syncthreads();                               // cnt is cleared again for the next channel of this block
    }
};

// out[c][2^B + 2]: codes 0 .. 2^B - 1, then below (code < 0) and above (code > 2^B - 1).  The code is uni_code of common.h, the value
// uni_bin clamps: an element inside the range lands on the code the fake-quantiser and the packers give it.
template <int B>
__global__ __launch_bounds__(TPB) void k_code_hist_uniform(const float* __restrict__ x, Geo g, const float* __restrict__ scale,
                                                           const float* __restrict__ zp, unsigned long long* __restrict__ out) {
    constexpr int NB = (1 << B) + 2;
    using Cn = Counters<NB>;
    __shared__ unsigned int cnt[Cn::WORDS];
    const float qmax = (float)((1 << B) - 1);
    for (int64_t c = blockIdx.y; c < g.n_ch; c += gridDim.y) {
        Cn::clear(cnt);
        const float s = scale[c], z = rintf(zp[c]);
        unsigned int* my = Cn::mine(cnt);
        stream_channel<false>(x, x, g, c, [&](float v, float) {
            const float cf = uni_code(v, s, z);
            // (a NaN is neither below nor above: it takes code 0, the code uni_bin gives it)
            const int bin = cf < 0.0f ? (1 << B) : cf > qmax ? (1 << B) + 1 : (int)fminf(fmaxf(cf, 0.0f), qmax);
            atomicAdd(my + bin, 1u);
        });
        Cn::flush(cnt, out + c * NB);
    }
}

// out[2^B + 1]: bins 0 .. 2^B - 1, then the masked code (the fake-quantiser's 255).  The bin is adalog_fq_bin of common.h, the function
// k_adalog (fakequant.hip) takes its ``bins`` output from.
template <int B>
__global__ __launch_bounds__(TPB) void k_code_hist_log(const float* __restrict__ x, Geo g, const float* __restrict__ scale,
                                                       const int64_t* __restrict__ q, const float* __restrict__ shift, int pre,
                                                       unsigned long long* __restrict__ out) {
    constexpr int NB = (1 << B) + 1;
    using Cn = Counters<NB>;
    __shared__ unsigned int cnt[Cn::WORDS];
    Cn::clear(cnt);
    const float s = scale[0], qf = (float)q[0], sh = shift ? shift[0] : 0.0f;
    const float inv_s = 1.0f / s, rq37 = 37.0f / qf;
    unsigned int* my = Cn::mine(cnt);
    stream_channel<false>(x, x, g, 0, [&](float v, float) {
        bool keep;
        const float k = adalog_fq_bin(v, s, inv_s, qf, rq37, shift != nullptr, sh, pre, 1 << B, keep);
        atomicAdd(my + (keep ? (int)k : (1 << B)), 1u);
    });
    Cn::flush(cnt, out);
}

// ------------------------------------------------------------------------------------------------ host
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

inline bool layout_ok(int64_t n, int64_t n_ch, int64_t inner) {
    return n >= 0 && n <= MAX_N && n_ch >= 1 && inner >= 1 && n_ch <= MAX_N && inner <= MAX_N / n_ch && n % (n_ch * inner) == 0;
}

// blocks per channel: about 1024 float4s (4 per thread) each, at most MAX_PARTS, about 8192 blocks over all channels, and never so
// few that a block's share reaches 2^31 elements
inline int parts_for(int64_t per_channel, int64_t n_ch) {
    int64_t p = (per_channel / 4 + 1023) / 1024;
    const int64_t cap = n_ch >= 8192 ? 1 : 8192 / n_ch;
    if (p > cap) p = cap;
    if (p > MAX_PARTS) p = MAX_PARTS;
    const int64_t need = (per_channel + (((int64_t)1 << 30) - 1)) >> 30;
    if (p < need) p = need;
    return (int)(p < 1 ? 1 : p);
}

inline bool cols_form(int64_t n_ch, int64_t inner) { return inner == 1 && n_ch > 1; }

// rows of the cols form a thread walks: about 64 per part
inline int cols_parts(int64_t rows, int64_t n_ch) {
    int64_t p = (rows + 63) / 64;
    const int64_t gx = (n_ch + TPB - 1) / TPB, cap = gx >= 8192 ? 1 : 8192 / gx;
    if (p > cap) p = cap;
    if (p > MAX_PARTS) p = MAX_PARTS;
    return (int)(p < 1 ? 1 : p);
}

inline int err_parts(int64_t n, int64_t n_ch, int64_t inner) {
    return cols_form(n_ch, inner) ? cols_parts(n / n_ch, n_ch) : parts_for(n / n_ch, n_ch);
}

inline Geo geo_for(int64_t n, int64_t n_ch, int64_t inner, const void* a, const void* b) {
    Geo g;
    g.inner = inner; g.n_ch = n_ch; g.rpc = n / (n_ch * inner);
    g.vec = (inner % 4 == 0) && aligned16(a) && (!b || aligned16(b));
    return g;
}

inline dim3 channel_grid(int parts, int64_t n_ch) { return dim3((unsigned)parts, (unsigned)(n_ch < 65535 ? n_ch : 65535)); }

// the two launches of err_stats / mean_err over accumulator A; ``what`` names the entry point in messages, ``label`` its kernels
template <class A>
int run_stats(const char* what, const char* label, const float* a, const float* b, int64_t n, int64_t n_channels, int64_t inner,
              double* out, void* workspace, int64_t workspace_bytes, hipStream_t st) {
    const int parts = err_parts(n, n_channels, inner);
    ADALOG_ARG_CHECK(workspace && ((uintptr_t)workspace & 7) == 0 &&
                         workspace_bytes >= n_channels * (int64_t)parts * A::N * (int64_t)sizeof(double),
                     "err_stats / mean_err: workspace missing, misaligned or smaller than the workspace query's answer");
    double* part = (double*)workspace;
    int rc;
    if (cols_form(n_channels, inner)) {
        const dim3 grid((unsigned)((n_channels + TPB - 1) / TPB), (unsigned)parts);
        rc = adalog_launch<k_stats_cols<A>>(label, 0, grid, TPB, 0, st, a, b, n / n_channels, n_channels, part);
    } else {
        rc = adalog_launch<k_stats<A>>(label, 0, channel_grid(parts, n_channels), TPB, 0, st, a, b, geo_for(n, n_channels, inner, a, b), part);
    }
    if (rc) return rc;
    ADALOG_LAUNCH_CHECK(what);
    const dim3 fgrid((unsigned)(n_channels < 4096 ? n_channels : 4096));
    rc = adalog_launch<k_stats_finish<A>>(label, 0, fgrid, TPB, 0, st, (const double*)part, n_channels, parts, out);
    if (rc) return rc;
    ADALOG_LAUNCH_CHECK(what);
    return 0;
}

}  // namespace

extern "C" int64_t adalog_err_stats_workspace_bytes(int64_t n, int64_t n_channels, int64_t inner) {
    if (!layout_ok(n, n_channels, inner)) return -1;
    if (n == 0) return 0;
    return n_channels * (int64_t)err_parts(n, n_channels, inner) * Acc::N * (int64_t)sizeof(double);
}

extern "C" int adalog_err_stats_f32(const float* a, const float* b, int64_t n, int64_t n_channels, int64_t inner, double* out,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
    ADALOG_ARG_CHECK(layout_ok(n, n_channels, inner), "err_stats: bad sizes (0 <= n <= 2^40, n a multiple of n_channels * inner)");
    ADALOG_ARG_CHECK(out && ((uintptr_t)out & 7) == 0, "err_stats: out must be an 8-byte aligned device pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        const hipError_t e = hipMemsetAsync(out, 0, (size_t)n_channels * Acc::N * sizeof(double), st);
        if (e != hipSuccess) { adalog_set_error("err_stats: hipMemsetAsync", e); return (int)e; }
        return 0;
    }
    ADALOG_ARG_CHECK(a && b && aligned4(a) && aligned4(b), "err_stats: a and b must be 4-byte aligned device pointers");
    return run_stats<Acc>("adalog_err_stats_f32", "k_err_stats", a, b, n, n_channels, inner, out, workspace, workspace_bytes, st);
}

// (one channel: the tensor is one contiguous run whatever ``inner`` says -- the form with the 16-byte loads)
extern "C" int64_t adalog_mean_err_workspace_bytes(int64_t n, int64_t n_channels, int64_t inner) {
    if (!layout_ok(n, n_channels, inner)) return -1;
    if (n == 0) return 0;
    if (n_channels == 1) inner = n;
    return n_channels * (int64_t)err_parts(n, n_channels, inner) * MeanAcc::N * (int64_t)sizeof(double);
}

extern "C" int adalog_mean_err_f32(const float* a, const float* b, int64_t n, int64_t n_channels, int64_t inner, double* out,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    ADALOG_ARG_CHECK(layout_ok(n, n_channels, inner), "mean_err: bad sizes (0 <= n <= 2^40, n a multiple of n_channels * inner)");
    ADALOG_ARG_CHECK(out && ((uintptr_t)out & 7) == 0, "mean_err: out must be an 8-byte aligned device pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        const hipError_t e = hipMemsetAsync(out, 0, (size_t)n_channels * MeanAcc::N * sizeof(double), st);
        if (e != hipSuccess) { adalog_set_error("mean_err: hipMemsetAsync", e); return (int)e; }
        return 0;
    }
    ADALOG_ARG_CHECK(a && b && aligned4(a) && aligned4(b), "mean_err: a and b must be 4-byte aligned device pointers");
    if (n_channels == 1) inner = n;
    return run_stats<MeanAcc>("adalog_mean_err_f32", "k_mean_err", a, b, n, n_channels, inner, out, workspace, workspace_bytes, st);
}

extern "C" int adalog_uniform_code_hist_f32(const float* x, int64_t n, const float* scale, const float* zero_point, int64_t n_channels,
                                            int64_t inner, int n_bits, int64_t* out, void* stream) {
    ADALOG_ARG_CHECK(n_bits >= 2 && n_bits <= 8, "uniform_code_hist: n_bits must be in [2,8]");
    ADALOG_ARG_CHECK(layout_ok(n, n_channels, inner), "uniform_code_hist: bad sizes (0 <= n <= 2^40, n a multiple of n_channels * inner)");
    ADALOG_ARG_CHECK(n_channels == 1 || inner >= 64, "uniform_code_hist: several channels need inner >= 64 (per-channel activations are not counted)");
    ADALOG_ARG_CHECK(scale && zero_point && out && ((uintptr_t)out & 7) == 0, "uniform_code_hist: null or misaligned pointer");
    ADALOG_ARG_CHECK(n == 0 || (x && aligned4(x)), "uniform_code_hist: x must be a 4-byte aligned device pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = ((int64_t)1 << n_bits) + 2;
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)(n_channels * nb) * sizeof(int64_t), st);
    if (e != hipSuccess) { adalog_set_error("uniform_code_hist: hipMemsetAsync", e); return (int)e; }
    if (n == 0) return 0;
    const Geo g = geo_for(n, n_channels, inner, x, nullptr);
    const dim3 grid = channel_grid(parts_for(n / n_channels, n_channels), n_channels);
    unsigned long long* o = (unsigned long long*)out;
    const int rc = adalog_dispatch<2, 3, 4, 5, 6, 7, 8>(n_bits, [&](auto b) {
        return adalog_launch<k_code_hist_uniform<decltype(b)::value>>("k_code_hist_uniform", 0, grid, TPB, 0, st, x, g, scale, zero_point, o);
    });
    if (rc) return rc;
    ADALOG_LAUNCH_CHECK("adalog_uniform_code_hist_f32");
    return 0;
}

extern "C" int adalog_log_code_hist_f32(const float* x, int64_t n, const float* scale, const int64_t* q, int n_bits, const float* shift,
                                        int pre, int64_t* out, void* stream) {
    ADALOG_ARG_CHECK(n_bits >= 2 && n_bits <= 8, "log_code_hist: n_bits must be in [2,8]");
    ADALOG_ARG_CHECK(n >= 0 && n <= MAX_N, "log_code_hist: n must be in [0, 2^40]");
    ADALOG_ARG_CHECK(scale && q && out && ((uintptr_t)out & 7) == 0, "log_code_hist: null or misaligned pointer");
    ADALOG_ARG_CHECK(n == 0 || (x && aligned4(x)), "log_code_hist: x must be a 4-byte aligned device pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = ((int64_t)1 << n_bits) + 1;
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)nb * sizeof(int64_t), st);
    if (e != hipSuccess) { adalog_set_error("log_code_hist: hipMemsetAsync", e); return (int)e; }
    if (n == 0) return 0;
    const Geo g = geo_for(n, 1, n, x, nullptr);
    const dim3 grid = channel_grid(parts_for(n, 1), 1);
    unsigned long long* o = (unsigned long long*)out;
    const int rc = adalog_dispatch<2, 3, 4, 5, 6, 7, 8>(n_bits, [&](auto b) {
        return adalog_launch<k_code_hist_log<decltype(b)::value>>("k_code_hist_log", 0, grid, TPB, 0, st, x, g, scale, q, shift, pre ? 1 : 0, o);
    });
    if (rc) return rc;
    ADALOG_LAUNCH_CHECK("adalog_log_code_hist_f32");
    return 0;
}
