// Operand packing for the candidate-scoring GEMMs (K7/K8/K11-K14 prologue).
//
// The reference re-materialises an fp32 fake-quantised copy of the searched operand for every candidate
// (quant_layers/linear.py:369-371,409-411,830-837; matmul.py:150-151,188-189,337-342; conv.py:240-242).  Here each
// operand is packed ONCE per scoring call into an MFMA-ready, K-contiguous compact image:
//   * uniformly quantised operands  -> int8   (q - z)                exact small integers  
//   * AdaLog operands               -> bf16   m * 2^-t               m = LUT numerator <= 4L-2, exact in bf16
//   * unquantised conv input        -> fp32   zero-padded copy
// so a candidate costs 1 B (2 B) per element instead of 4 B x ~8 temporaries, and the de-quantisation scales are
// applied once per output in the GEMM epilogue.  Output layout: out[c][g][r][Kp], Kp = K rounded up to 64 bytes,
// zero padded (zeros contribute nothing to the integer dot product).
#include "common.h"
#include "softmax_adalog.h"
#include <hip/hip_bf16.h>
#include <type_traits>
#include <stdlib.h>

namespace {

enum { KIND_UNIFORM = 0, KIND_ADALOG = 1, KIND_RAW = 2 };

struct PackArgs {
    const float* x;
    int64_t G, R, K, sxg, sxr, sxk;
    // parameter addressing: idx = c*pc + (g % gmod)*pg + r*pr
    const float* scale;
    const float* zp;      // uniform: zero point (rounded in-kernel); adalog: unused
    const float* qv;      // adalog: log-base numerator q per candidate (same addressing, pr ignored)
    int64_t C, pc, gmod, pg, pr;
    float qmax;           // 2L-1
    int levels2;          // 2L
    const float* mant;    // adalog: 37 integer numerators of the search table (linear.py:750-752)
    const float* shift;   // adalog: optional input shift (post-GELU), device scalar
    int clamp_u;          // adalog: clamp((x+shift)/s, 1e-15, 1) (linear.py:830) or raw log2 (matmul.py:337)
    void* out;
    int64_t Kp;
    int32_t* rowsum;      // optional [C][G][R] sum_k (q - z)
    int c_inner;          // 0: out[c][g][r][Kp]   1: out[g][r][c][Kp] (candidates innermost: GEMM columns = (row, candidate))
    int pre;              // adalog, fast kernel: 1 = the operand is GELU(x) (erf form, ATen's expression): quant_forward of fc2 reads fc1's output
};

// x * 0.5 * (1 + erf(x / sqrt 2)) as ATen's GeluCUDAKernelImpl evaluates it in fp32 ("none" approximation)
__device__ __forceinline__ float gelu_erf(float x) { return (x * 0.5f) * (1.0f + erff(x * 0.70710678118654752440f)); }

struct fp8_t { uint8_t b; };   // e4m3 byte as the hardware converts it (v_cvt_pk_fp8_f32); integers up to 16 are exact

template <typename T> struct Out;
template <> struct Out<int8_t> { static constexpr int EPT = 16; };
template <> struct Out<fp8_t> { static constexpr int EPT = 16; };
template <> struct Out<__hip_bfloat16> { static constexpr int EPT = 8; };
template <> struct Out<float> { static constexpr int EPT = 4; };

template <typename T> __device__ __forceinline__ T cvt(float v);
template <> __device__ __forceinline__ int8_t cvt<int8_t>(float v) { return (int8_t)(int)v; }
template <> __device__ __forceinline__ fp8_t cvt<fp8_t>(float v) {
    fp8_t r; r.b = (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(v, 0.0f, 0, false) & 0xff); return r;
}
template <> __device__ __forceinline__ __hip_bfloat16 cvt<__hip_bfloat16>(float v) { return __float2bfloat16(v); }
template <> __device__ __forceinline__ float cvt<float>(float v) { return v; }

// ---- the pieces the K-contiguous packers below share

// Row of the output image that (candidate c, group g, row r) writes: [c][g][r], or [g][r][c] with the candidates innermost (c_inner).
__device__ __forceinline__ int64_t out_row(const PackArgs& a, int64_t g, int64_t r, int64_t c) {
    return a.c_inner ? (g * a.R + r) * a.C + c : (c * a.G + g) * a.R + r;
}
// Elements from candidate c to candidate c + cstep of the same (g, r): what a loop over the candidates adds to its output pointer.
__device__ __forceinline__ int64_t out_step(const PackArgs& a, int64_t cstep) {
    return (a.c_inner ? cstep : cstep * a.G * a.R) * a.Kp;
}

// xv[0..3] = elements k0 .. k0 + 3 of a row of K elements (xp points at element k0), zeros from K on: one 16-byte load when the quad is
// whole and aligned, otherwise only the elements below K are read.
__device__ __forceinline__ void load_quad(const float* xp, int64_t k0, int64_t K, float* xv) {
    if (k0 + 3 < K && ((uintptr_t)xp & 15) == 0) {
        const float4 v = *reinterpret_cast<const float4*>(xp);
        xv[0] = v.x; xv[1] = v.y; xv[2] = v.z; xv[3] = v.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[e] = (k0 + e < K) ? xp[e] : 0.0f;
    }
}

// A uniform quantiser as the fast packers use it: {1/s, s, lo, hi} with z = rne(zero point), lo = -z, hi = qmax - z, so that
// clamp(k + z, 0, qmax) - z == med3(k, lo, hi).
__device__ __forceinline__ float4 uni_par(float s, float zp, float qmax) {
    const float z = rintf(zp);
    return make_float4(__builtin_amdgcn_rcpf(s), s, -z, qmax - z);
}
__device__ __forceinline__ float uni_clamp(float k, const float4& par) { return __builtin_amdgcn_fmed3f(k, par.z, par.w); }

// k[e] = rne(x[e] / s), the reference's round(x / s), for N elements at the price of a multiplication each: t = x * (1/s) is within
// 1.8e-7 * |t| of x / s, i.e. < 1e-4 wherever the clamp does not decide anyway (|t| < 555), so rne(t) is the answer unless some t lies
// within 1e-4 of a rounding tie.  Then (rare) the IEEE quotient decides for all N: outside the tie zone both round alike.
template <int N>
__device__ __forceinline__ void uni_codes(const float* x, const float4& par, float* k) {
    float dm = 0.0f;
#pragma unroll
    for (int e = 0; e < N; ++e) { const float t = x[e] * par.x; k[e] = rintf(t); dm = fmaxf(dm, fabsf(t - k[e])); }
    if (__builtin_expect(dm > 0.4999f, 0)) {
#pragma unroll
        for (int e = 0; e < N; ++e) k[e] = rintf(x[e] / par.y);
    }
}

// Four codes (small integers: exact in every output type) as the 32-bit word a one-byte type stores.  fp8: the hardware's e4m3
// conversion; int8: (v + 128) saturates into a byte lane per instruction, xor 0x80 turns it into two's complement.
template <typename T>
__device__ __forceinline__ unsigned code_word(const float* v) {
    static_assert(sizeof(T) == 1, "one-byte outputs");
    if (std::is_same<T, fp8_t>::value) {
        const int pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
        return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], pk, true);
    }
    unsigned pk = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) pk = __builtin_amdgcn_cvt_pk_u8_f32(v[e] + 128.0f, e, pk);
    return pk ^ 0x80808080u;
}
// ... and written to op in any output type: one 4-, 8- (bf16: the top halves of the fp32) or 16-byte store.
template <typename T>
__device__ __forceinline__ void store_quad(T* op, const float* v) {
    if constexpr (sizeof(T) == 1) {
        *reinterpret_cast<unsigned*>(op) = code_word<T>(v);
    } else if constexpr (sizeof(T) == 2) {
        const unsigned b0 = __float_as_uint(v[0]), b1 = __float_as_uint(v[1]), b2 = __float_as_uint(v[2]), b3 = __float_as_uint(v[3]);
        *reinterpret_cast<uint2*>(op) = make_uint2((b0 >> 16) | (b1 & 0xffff0000u), (b2 >> 16) | (b3 & 0xffff0000u));
    } else {
        *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// rowsum[ridx] += v over the lanes of a wave.  `wave`, the same in every lane: all 64 lanes are here and their rows are at most two
// (lane 0's and one other) -- then each row's lanes are reduced in the wave and one lane per row adds; a lane with ridx < 0 has nothing
// to add.  Otherwise every lane adds for itself.  (Integer sums: the order of the atomics does not show.)
__device__ __forceinline__ void row_sum(int32_t* rowsum, int ridx, int v, bool wave) {
    if (!wave) {
        if (ridx >= 0 && v != 0) atomicAdd(rowsum + ridx, v);
        return;
    }
    const int first = __builtin_amdgcn_readfirstlane(ridx);
    const bool live = ridx >= 0, mine = ridx == first;
    const int lane = threadIdx.x & 63;
    int s1 = (live && mine) ? v : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s1 += __shfl_xor(s1, o);
    if (lane == 0 && first >= 0 && s1 != 0) atomicAdd(rowsum + first, s1);
    const unsigned long long other = __ballot(live && !mine);
    if (other) {                                                             // (the same in every lane)
        int s2 = (live && !mine) ? v : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
        const int ol = __ffsll((long long)other) - 1;
        const int r2 = __shfl(ridx, ol);
        if (lane == ol && s2 != 0) atomicAdd(rowsum + r2, s2);
    }
}

template <typename T, int KIND, bool RFAST>
__global__ __launch_bounds__(256) void k_pack(PackArgs a) {
    constexpr int EPT = Out<T>::EPT;
    const int64_t nchunk = a.Kp / EPT;
    const int64_t per_c = a.G * a.R * nchunk;
    const int64_t c = blockIdx.y;
    __shared__ float s_mant[ADALOG_R];
    if (KIND == KIND_ADALOG) {
        if (threadIdx.x < ADALOG_R) s_mant[threadIdx.x] = a.mant[threadIdx.x];
        __syncthreads();
    }
    const float sh = (KIND == KIND_ADALOG && a.shift) ? a.shift[0] : 0.0f;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < per_c; idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t g, r, ch;
        if (RFAST) {
            r = idx % a.R;
            int64_t t = idx / a.R;
            ch = t % nchunk;
            g = t / nchunk;
        } else {
            ch = idx % nchunk;
            int64_t t = idx / nchunk;
            r = t % a.R;
            g = t / a.R;
        }
        const int64_t pidx = c * a.pc + (g % a.gmod) * a.pg + r * a.pr;
        float s = 1.0f, z = 0.0f, qf = 37.0f;
        if (KIND != KIND_RAW) s = a.scale[pidx];
        if (KIND == KIND_UNIFORM) z = rintf(a.zp[pidx]);
        if (KIND == KIND_ADALOG) qf = a.qv[c * a.pc + (g % a.gmod) * a.pg];
        const float* xp = a.x + g * a.sxg + r * a.sxr;
        alignas(16) T vals[EPT];
        int isum = 0;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int64_t k = ch * EPT + e;
            float v = 0.0f;
            if (k < a.K) {
                const float xv = xp[k * a.sxk];
                if (KIND == KIND_UNIFORM) {
                    v = fminf(fmaxf(rintf(xv / s) + z, 0.0f), a.qmax) - z;
                    isum += (int)v;
                } else if (KIND == KIND_ADALOG) {
                    float u = (a.shift ? xv + sh : xv) / s;
                    if (a.clamp_u) u = fminf(fmaxf(u, 1e-15f), 1.0f);
                    float kk = adalog_k(u, qf);
                    if (kk < (float)a.levels2 && kk == kk) {        // masked bins (and NaN) -> 0
                        kk = fmaxf(kk, 0.0f);
                        const int kq = (int)kk * (int)qf;             // exact: k <= 255, q <= 137
                        const int t = kq / ADALOG_R, j = kq - t * ADALOG_R;
                        v = (t > 100) ? 0.0f : ldexpf(s_mant[j], -t);  // < 2^-100: below fp32 resolution of the sums
                    }
                } else {
                    v = xv;
                }
            }
            vals[e] = cvt<T>(v);
        }
        T* op = reinterpret_cast<T*>(a.out) + out_row(a, g, r, c) * a.Kp + ch * EPT;
        *reinterpret_cast<uint4*>(op) = *reinterpret_cast<const uint4*>(vals);
        if (KIND == KIND_UNIFORM && a.rowsum) atomicAdd(a.rowsum + (c * a.G + g) * a.R + r, isum);
    }
}

// K-contiguous sources (activations, weights, q@k^T operands): one thread owns 4 consecutive k of one row and loops over
// ALL candidates, so the fp32 source is read once (coalesced float4) instead of once per candidate, and every store
// instruction of a wave writes one contiguous 256 B / 512 B / 1 KiB run.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void k_pack_kfast(PackArgs a) {
    static_assert(KIND == KIND_UNIFORM || KIND == KIND_RAW, "AdaLog operands: k_pack_adalog_fast, or k_pack");
    const int64_t nq = a.Kp >> 2;
    const int64_t total = a.G * a.R * nq;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t kq = idx % nq;
        const int64_t t0 = idx / nq;
        const int64_t r = t0 % a.R, g = t0 / a.R;
        const int64_t k0 = kq << 2;
        float xv[4];
        load_quad(a.x + g * a.sxg + r * a.sxr + k0, k0, a.K, xv);
        const bool full = k0 + 3 < a.K;
        const int64_t pbase = (g % a.gmod) * a.pg + r * a.pr;
        // (uniform: the next candidate's scale and zero point are fetched under the current one's arithmetic -- with per-row
        // parameters each iteration otherwise starts with an L2 round trip: 1.8 TB/s written for the fc2 weight candidates)
        float s_nx = 1.0f, z_nx = 0.0f;
        if (KIND == KIND_UNIFORM && (int64_t)blockIdx.y < a.C) { s_nx = a.scale[blockIdx.y * a.pc + pbase]; z_nx = a.zp[blockIdx.y * a.pc + pbase]; }
        for (int64_t c = blockIdx.y; c < a.C; c += gridDim.y) {
            float v[4];
            if (KIND == KIND_RAW) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = xv[e];
            } else {
                // per element: mul, rint, sub, max, med3 [, add, cvt_pk_u8]
                const float4 par = uni_par(s_nx, z_nx, a.qmax);
                if (c + gridDim.y < a.C) { s_nx = a.scale[(c + gridDim.y) * a.pc + pbase]; z_nx = a.zp[(c + gridDim.y) * a.pc + pbase]; }
                float k[4];
                uni_codes<4>(xv, par, k);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (full || k0 + e < a.K) ? uni_clamp(k[e], par) : 0.0f;
            }
            store_quad<T>(reinterpret_cast<T*>(a.out) + out_row(a, g, r, c) * a.Kp + k0, v);
            if (KIND == KIND_UNIFORM && a.rowsum) {
                // one atomic per wavefront when all 64 lanes work on the same row (the common case: Kp/4 >= 64)
                const int ridx = (int)((c * a.G + g) * a.R + r);
                const bool one_row = __all(ridx == __builtin_amdgcn_readfirstlane(ridx)) && __popcll(__ballot(1)) == 64;
                row_sum(a.rowsum, ridx, (int)((v[0] + v[1]) + (v[2] + v[3])), one_row);   // small integers: exact in fp32
            }
        }
    }
}

// AdaLog packing, per-tensor scale (pg == 0), K-contiguous source: the hot form (post-GELU and post-softmax
// searches write 2.5 GB of bf16 per call).  Everything that depends only on the candidate -- the value LUT, 37/q,
// log2(s)*37/q, the clamp bound -- is built once per block in LDS, so a candidate costs per element
//   fma, med3, rndne, sub, cmp(tie zone), cvt, address, ds_read_u16   (+ 1/2 v_perm, 1/4 store).
// Bins >= 2L and x <= 0 without the u-clamp read one of two zero entries behind each LUT row, so no select is needed.
__global__ __launch_bounds__(256) void k_pack_adalog_fast(PackArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int lw = a.levels2 + 2;
    float4* s_par = reinterpret_cast<float4*>(s_raw);                       // [C] {37/q, log2(s)*37/q, lower, upper}
    unsigned short* s_lut = reinterpret_cast<unsigned short*>(s_raw + (size_t)a.C * sizeof(float4));   // [C][2L + 2]
    const float NL15 = 49.828921f;                                           // -fl32(log2(1e-15f))
    for (int e = threadIdx.x; e < (int)a.C * lw; e += blockDim.x) {
        const int c = e / lw, k = e - c * lw;
        const int kqv = k * (int)a.qv[c * a.pc];
        const int t = kqv / ADALOG_R, j = kqv - t * ADALOG_R;
        const float v = (k >= a.levels2 || t > 100) ? 0.0f : ldexpf(a.mant[j], -t);
        s_lut[e] = (unsigned short)(__float_as_uint(v) >> 16);              // exact: <= 8 significant bits
    }
    for (int c = threadIdx.x; c < (int)a.C; c += blockDim.x) {
        const float s = a.scale[c * a.pc], qf = a.qv[c * a.pc];
        const float rq37 = 37.0f / qf;
        const float top = (float)a.levels2 + 0.75f;                          // rounds to 2L + 1: a zero entry
        s_par[c] = make_float4(rq37, __log2f(s) * rq37, a.clamp_u ? 0.0f : -0.25f,
                               a.clamp_u ? fminf(NL15 * rq37, top) : top);
    }
    __syncthreads();
    const float sh = a.shift ? a.shift[0] : 0.0f;
    const int64_t nq = a.Kp >> 2;
    const int64_t total = a.G * a.R * nq;
    const int64_t cstep = gridDim.y;
    const bool ragged = (a.K & 3) != 0;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t kq = idx % nq;
        const int64_t t0 = idx / nq;
        const int64_t r = t0 % a.R, g = t0 / a.R;
        const int64_t k0 = kq << 2;
        float xv[4] = {0.f, 0.f, 0.f, 0.f};
        const int nlive = (int)min((int64_t)4, max((int64_t)0, a.K - k0));   // data elements of this quad (rest: zero padding)
        const bool live = nlive > 0;
        if (live) {
            load_quad(a.x + g * a.sxg + r * a.sxr + k0, k0, a.K, xv);
            if (a.pre == 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) xv[e] = gelu_erf(xv[e]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e < nlive) xv[e] += sh;
        }
        float lx[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            lx[e] = __log2f(xv[e]);                                          // -inf for 0, NaN for negatives
            if (!(lx[e] == lx[e])) lx[e] = -__builtin_inff();                // x < 0: u clamps to 1e-15 / bin masked, like x = 0
        }
        const int64_t c0 = blockIdx.y;
        const int64_t ostep = out_step(a, cstep);
        __hip_bfloat16* op = reinterpret_cast<__hip_bfloat16*>(a.out) + out_row(a, g, r, c0) * a.Kp + k0;
        for (int64_t c = c0; c < a.C; c += cstep, op += ostep) {
            uint2 pk = make_uint2(0u, 0u);
            if (live) {
                const float4 pr = s_par[c];
                const unsigned short* lut = s_lut + c * lw;
                unsigned short hv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // (log2 s - log2 x) * 37/q, one explicit fma: this value only steers the fast path (the tie zone covers its error)
                    const float t = __builtin_amdgcn_fmed3f(__builtin_fmaf(-lx[e], pr.x, pr.y), pr.z, pr.w);
                    float kk = rintf(t);
                    // within 1e-4 of a rounding tie the fast t (error ~1e-5 below 2L + 1) does not decide: exact path.
                    // One lane taking it stalls the wave, so the zone is as narrow as the error bound allows.
                    if (__builtin_expect(fabsf(t - kk) > 0.4999f, 0)) {
                        const float s = a.scale[c * a.pc], qf = a.qv[c * a.pc];
                        float ue = xv[e] / s;
                        if (a.clamp_u) ue = fminf(fmaxf(ue, 1e-15f), 1.0f);
                        kk = adalog_k(ue, qf);
                        kk = (kk == kk) ? fminf(fmaxf(kk, 0.0f), (float)(a.levels2 + 1)) : (float)(a.levels2 + 1);
                    }
                    hv[e] = lut[(int)kk];
                }
                if (ragged) {                                                // K % 4 != 0: the row's last quad is part padding
#pragma unroll
                    for (int e = 1; e < 4; ++e) if (e >= nlive) hv[e] = 0;
                }
                pk = make_uint2((unsigned)hv[0] | ((unsigned)hv[1] << 16), (unsigned)hv[2] | ((unsigned)hv[3] << 16));
            }
            *reinterpret_cast<uint2*>(op) = pk;
        }
    }
}

// Uniform int8 packing with per-tensor candidates (pg == pr == 0: the activation searches, 0.3-1.2 GB per call): the
// candidate's reciprocal scale and clamp bounds come from LDS; per element  mul, rndne, sub, max (tie zone), add, med3,
// cvt_pk_u8;  the output pointer advances by a constant per candidate.
template <bool FP8>
__global__ __launch_bounds__(256) void k_pack_uniform_i8_fast(PackArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    float4* s_par = reinterpret_cast<float4*>(s_raw);                       // [C] {1/s, s, -z + bias, qmax - z + bias}
    const float vbias = FP8 ? 0.0f : 128.0f;                                 // int8 goes through a biased u8 conversion
    // per-group parameters (pg != 0: one (scale, zp) per candidate and head): grid.z walks the groups, so a block's
    // parameters are still one LDS table
    const bool per_group = a.pg != 0;
    const int64_t pgo = per_group ? ((int64_t)blockIdx.z % a.gmod) * a.pg : 0;
    for (int c = threadIdx.x; c < (int)a.C; c += blockDim.x) {
        float4 par = uni_par(a.scale[c * a.pc + pgo], a.zp[c * a.pc + pgo], a.qmax);
        par.z += vbias; par.w += vbias;
        s_par[c] = par;
    }
    __syncthreads();
    const int64_t nq = a.Kp >> 2;
    const int64_t total = (per_group ? 1 : a.G) * a.R * nq;
    const int64_t cstep = gridDim.y;
    const bool ragged = (a.K & 3) != 0;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t kq = idx % nq;
        const int64_t t0 = idx / nq;
        const int64_t r = t0 % a.R, g = per_group ? (int64_t)blockIdx.z : t0 / a.R;
        const int64_t k0 = kq << 2;
        float xv[4];
        const int nlive = (int)min((int64_t)4, max((int64_t)0, a.K - k0));
        const bool live = nlive > 0;
        load_quad(a.x + g * a.sxg + r * a.sxr + k0, k0, a.K, xv);
        const int64_t c0 = blockIdx.y;
        const int64_t ostep = out_step(a, cstep);
        int8_t* op = reinterpret_cast<int8_t*>(a.out) + out_row(a, g, r, c0) * a.Kp + k0;
        for (int64_t c = c0; c < a.C; c += cstep, op += ostep) {
            unsigned pk = FP8 ? 0u : 0x80808080u;                             // (biased) zeros
            if (live) {
                const float4 pr = s_par[c];
                float k[4], vb[4];
                uni_codes<4>(xv, pr, k);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    vb[e] = uni_clamp(k[e] + vbias, pr);                      // int8: (q - z) + 128 in [1, 255]
                    if (ragged && e >= nlive) vb[e] = vbias;
                }
                if (FP8) {
                    pk = code_word<fp8_t>(vb);
                } else {
                    pk = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) pk = __builtin_amdgcn_cvt_pk_u8_f32(vb[e], e, pk);
                }
            }
            *reinterpret_cast<unsigned*>(op) = FP8 ? pk : pk ^ 0x80808080u;   // int8: un-bias to two's complement
        }
    }
}

// Uniform packing with per-ROW candidate parameters (pr != 0: the weight candidates of every weight search -- a (scale, zero
// point) per candidate and output channel).  k_pack_kfast fetches the two parameters of every (candidate, row) from global
// memory inside the candidate loop; even fetched one candidate ahead that is an L2 round trip per iteration, and the fc2
// weight candidates (128 x 384 x 1536 bf16 = 151 MB) were written at 1.05 TB/s.  Here a block owns 256 consecutive k-quads
// (at most TAB_ROWS rows), stages {1/s, s, -z, qmax - z} of those rows for ALL candidates in LDS once, and its loop over the
// candidates touches global memory only to store.  The tie zone is tested once per thread and candidate.
// W = 4 k per thread: any output type, ragged K.  W = 16, one-byte outputs only: one 16-byte store per lane and candidate (1 KiB per
// wave-store; 4-byte stores wrote the fc2 weight candidates -- 75 MB of fp8 per launch -- at 1.4 TB/s); needs K % 16 == 0 == Kp % 16 (a
// thread's 16 are all data or all padding) and 16-byte aligned rows.  Both need Kp / W >= 64: a wave then spans at most two rows, whose
// sums are reduced per row inside the wave, and a block at most 256 / (Kp / W) + 2 <= TAB_ROWS.
constexpr int TAB_ROWS = 6;
template <typename T, int W>
__global__ __launch_bounds__(256) void k_pack_uniform_tab(PackArgs a) {
    static_assert(W == 4 || (W == 16 && sizeof(T) == 1), "16 k per thread: one-byte outputs");
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    float4* s_tab = reinterpret_cast<float4*>(s_raw);                       // [rows of this block][C]
    const int64_t nq = a.Kp / W;                                             // W-element pieces per row
    const int64_t total = a.G * a.R * nq;
    const int64_t q0 = (int64_t)blockIdx.x * 256;
    const int64_t row0 = q0 / nq;                                            // flattened (g, r) row
    const int64_t rowN = min((q0 + 255) / nq, a.G * a.R - 1);
    const int nrows = (int)(rowN - row0 + 1);
    const int C = (int)a.C;
    for (int e = threadIdx.x; e < nrows * C; e += 256) {
        const int rl = e / C, c = e - rl * C;
        const int64_t gr = row0 + rl, g = gr / a.R, r = gr - g * a.R;
        const int64_t pidx = c * a.pc + (g % a.gmod) * a.pg + r * a.pr;
        s_tab[e] = uni_par(a.scale[pidx], a.zp[pidx], a.qmax);
    }
    __syncthreads();
    // the last block's threads beyond the operand stay (the row sums are reduced by whole waves): no data, no store
    const int64_t idx = q0 + threadIdx.x;
    const bool live = idx < total;
    const int64_t gr = live ? idx / nq : row0, kq = live ? idx - gr * nq : 0;
    const int64_t g = gr / a.R, r = gr - g * a.R;
    const int64_t k0 = kq * W, K = live ? a.K : 0;
    const float* xp = a.x + g * a.sxg + r * a.sxr + k0;
    const bool full = k0 + W <= K;
    float xv[W];
    if constexpr (W == 16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 x4 = full ? reinterpret_cast<const float4*>(xp)[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            xv[4 * j] = x4.x; xv[4 * j + 1] = x4.y; xv[4 * j + 2] = x4.z; xv[4 * j + 3] = x4.w;
        }
    } else {
        load_quad(xp, k0, K, xv);
    }
    const float4* tab = s_tab + (int)(gr - row0) * C;
    const int64_t cstep = gridDim.y;
    T* op = reinterpret_cast<T*>(a.out) + out_row(a, g, r, blockIdx.y) * a.Kp + k0;
    for (int64_t c = blockIdx.y; c < a.C; c += cstep, op += out_step(a, cstep)) {
        const float4 par = tab[c];
        float k[W], v[W];
        uni_codes<W>(xv, par, k);
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = (full || (W == 4 && k0 + e < K)) ? uni_clamp(k[e], par) : 0.0f;
        if (live) {
            if constexpr (W == 16) *reinterpret_cast<uint4*>(op) = make_uint4(code_word<T>(v), code_word<T>(v + 4), code_word<T>(v + 8), code_word<T>(v + 12));
            else store_quad<T>(op, v);
        }
        if (a.rowsum) {
            float fs = v[0];                                                 // small integers: exact in fp32
#pragma unroll
            for (int e = 1; e < W; ++e) fs += v[e];
            row_sum(a.rowsum, live ? (int)((c * a.G + g) * a.R + r) : -1, (int)fs, true);
        }
    }
}

// quant_forward of softmax . v (reference utils/wrap_net.py:26-30 + quant_layers/matmul.py:43-45): (scores * scale).softmax(-1) and the
// AdaLog quantisation of the probabilities in ONE pass -- the probabilities are never written; the output is the packed bf16
// operand of the product (what k_pack_adalog_fast writes for C = 1).  A wavefront owns a row of S <= 256 scores.  The arithmetic is
// ATen's softmax_warp_forward, operation for operation (element k = lane + 64 it; max; e = exp(x - max) summed per lane in `it`
// order, then the xor butterfly 32, 16, .., 1; e / sum), so that the composed route (torch softmax, then the packer) and this
// kernel quantise the same fp32 probabilities.
//
// BIAS (Swin's window attention, reference utils/wrap_net.py:35-52): no multiplier; instead the relative-position bias is gathered and
// the shift mask added in front of the softmax, as the module route's separate ATen adds round them: e = s + table[index[r][c]][h],
// then e = e + mask[w][r][c] -- rows [G = windows * H][S][S], h = g % H, w = (g / H) % nW.
struct SoftmaxPackArgs {
    const float* x; int64_t rows; int S; float mul;      // scores [rows][S] (contiguous), multiplied by `mul` first
    const float* scale; const float* qv; const float* mant; int levels2;   // the AdaLog quantiser: device scalars (scale, q), 37 numerators
    unsigned short* out; int64_t Kp;                     // bf16 bits [rows][Kp], zero beyond S
    const float* table; const int64_t* index;            // BIAS: relative_position_bias_table [*][H], relative_position_index [S][S]
    const float* mask; int H, nW;                        // BIAS: shift mask [nW][S][S] or null
};
constexpr int SM_ROWS = 4;
// NS slots per lane (softmax_adalog.h: 4 for S <= 256, 8 for S <= 512, 16 for S <= 1024), ROWS rows per wavefront: the long-row forms take
// fewer rows at a time so that the loads in flight stay at 16 per lane
template <bool BIAS, int NS = 4, int ROWS = SM_ROWS>
__global__ __launch_bounds__(256) void k_softmax_adalog_pack_t(SoftmaxPackArgs a) {
    __shared__ unsigned short s_lut[258];
    const float qf = a.qv[0], sc = a.scale[0];
    adalog_value_lut_bf16(s_lut, a.levels2, qf, a.mant);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const float inv_s = __builtin_amdgcn_rcpf(sc), rq37 = 37.0f / qf;
    // a wavefront takes ROWS consecutive rows (the table above is built once per 4 ROWS rows); their loads are issued together
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS;
    float raw[ROWS][NS];
#pragma unroll
    for (int rr = 0; rr < ROWS; ++rr) {
        const bool rv = row0 + rr < a.rows;
        const float* xr = a.x + (rv ? row0 + rr : 0) * a.S;
#pragma unroll
        for (int it = 0; it < NS; ++it) {
            const int k = lane + 64 * it;
            raw[rr][it] = (rv && k < a.S) ? xr[k] : 0.0f;
        }
    }
#pragma unroll
    for (int rr = 0; rr < ROWS; ++rr) {
        const int64_t row = row0 + rr;
        if (row >= a.rows) return;
        float el[NS];
        if constexpr (BIAS) {
            const int64_t g = row / a.S;
            const int r = (int)(row - g * a.S), h = (int)(g % a.H);
            const int64_t* ix = a.index + (int64_t)r * a.S;
            const float* mk = a.mask ? a.mask + ((g / a.H) % a.nW * a.S + r) * a.S : nullptr;
#pragma unroll
            for (int it = 0; it < NS; ++it) {
                const int k = lane + 64 * it;
                float e = -__builtin_inff();
                if (k < a.S) {
                    e = raw[rr][it] + a.table[ix[k] * a.H + h];
                    if (mk) e = e + mk[k];
                }
                el[it] = e;
            }
        } else {
#pragma unroll
            for (int it = 0; it < NS; ++it) el[it] = lane + 64 * it < a.S ? raw[rr][it] * a.mul : -__builtin_inff();
        }
        const float sum = softmax_warp_row(el);
        unsigned short* orow = a.out + row * a.Kp;
#pragma unroll
        for (int it = 0; it < NS; ++it) {
            const int k = lane + 64 * it;
            if (k >= a.Kp) break;
            unsigned short hv = 0;
            if (k < a.S) hv = adalog_prob_bf16(el[it], sum, sc, inv_s, qf, rq37, a.levels2, s_lut);
            orow[k] = hv;
        }
        if constexpr (NS > 4) {                                        // a Kp past the slots of this form: zero columns
            for (int64_t k = lane + 64 * NS; k < a.Kp; k += 64) orow[k] = 0;
        }
    }
}

// quant_forward of an attention block (reference utils/wrap_net.py:19-31 + quant_layers/matmul.py:43-45): the qkv projection's output
// [B][N][3][H][D] is split into heads, passed through the three per-head uniform input quantisers (q and k of q . k^T, v of
// softmax . v) and written as the packed operands of the two products in ONE pass -- no permuted fp32 copies of q / k / v, no three
// packer launches:  qp, kp int8 [B*H][N][128] (D codes q - z, 128 - D zero bytes), vp bf16 [B*H][D][Np] (v transposed: a row per
// channel, a column per token, zero beyond N).  Codes as adalog_pack_uniform writes them: clamp(rne(x / s) + rne(z), 0, qmax) - rne(z).
// D = 16 QD (QD = 1..4): a block takes 64 tokens of one (image, head), QD threads per token (16 channels each); the other threads of
// the block only help with the transposed store of v.  QMUL (Swin, wrap_net.py:41): q is multiplied by q_mul first (fp32 product,
// ATen's q * scale with the scale cast to fp32) -- the codes are those of the module route's pack of q * scale.
struct AttnSplitArgs {
    const float* qkv; int B, N, H;
    const float* qs; const float* qz; const float* ks; const float* kz; const float* vs; const float* vz;    // [H] each (pg = 1) or [1] (pg = 0)
    int pg; float q_qmax, k_qmax, v_qmax;
    int8_t* qp; int8_t* kp; unsigned short* vp; int64_t Np;
    float q_mul;
};
template <int QD, bool QMUL>
__global__ __launch_bounds__(256) void k_attn_split_pack(AttnSplitArgs a) {
    constexpr int D = 16 * QD;
    __shared__ unsigned short vt[64][72];                       // [channel][token of the tile], rows padded against bank conflicts
    const int h = blockIdx.y, b = blockIdx.z, n0 = blockIdx.x * 64;
    const int t = threadIdx.x, row = t / QD, qt = t % QD;      // token of the tile, 16-channel slice
    const bool loader = t < 64 * QD;                           // (QD = 4: every thread)
    const int n = n0 + row;
    const int HD = a.H * D;
    const int64_t g = (int64_t)b * a.H + h;
    const int pi = a.pg ? h : 0;
    const bool live = loader && n < a.N;
    const float* src = a.qkv + ((int64_t)b * a.N + (live ? n : 0)) * (3 * HD) + h * D + qt * 16;
    auto load16 = [&](const float* p_, float (&x)[16]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 v = *reinterpret_cast<const float4*>(p_ + 4 * j);
            x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w;
        }
    };
    auto codes = [&](const float (&x)[16], float s, float z, float qmax, float (&c)[16]) {
#pragma unroll
        for (int e = 0; e < 16; ++e) c[e] = fminf(fmaxf(rintf(x[e] / s) + z, 0.0f), qmax) - z;
    };
    float x[16], c[16];
    // q and k: one 16-byte store of codes and (128 - D) / 16 / QD of padding per thread and operand
    for (int which = 0; which < 2; ++which) {
        const float s = which ? a.ks[pi] : a.qs[pi], z = rintf(which ? a.kz[pi] : a.qz[pi]), qmax = which ? a.k_qmax : a.q_qmax;
        if (live) {
            load16(src + which * HD, x);
            if constexpr (QMUL) {
                if (which == 0) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) x[e] = x[e] * a.q_mul;
                }
            }
            codes(x, s, z, qmax, c);
            uint4 o;
            unsigned* ow = reinterpret_cast<unsigned*>(&o);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned pk = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) pk |= ((unsigned)(int)c[4 * j + e] & 0xffu) << (8 * e);
                ow[j] = pk;
            }
            int8_t* dst = (which ? a.kp : a.qp) + (g * a.N + n) * 128;
            *reinterpret_cast<uint4*>(dst + qt * 16) = o;
#pragma unroll
            for (int zc = QD + qt; zc < 8; zc += QD) *reinterpret_cast<uint4*>(dst + zc * 16) = make_uint4(0, 0, 0, 0);
        }
    }
    // v: quantise, transpose through LDS, rows of 64 tokens (128 bytes) out
    {
        const float s = a.vs[pi], z = rintf(a.vz[pi]);
        if (live) { load16(src + 2 * HD, x); codes(x, s, z, a.v_qmax, c); }
        if (loader) {
#pragma unroll
            for (int e = 0; e < 16; ++e) vt[qt * 16 + e][row] = live ? (unsigned short)(__float_as_uint(c[e]) >> 16) : (unsigned short)0;   // small integers: exact in bf16
        }
        __syncthreads();
        const int ch = t >> 2, tq = t & 3;                       // channel, 16-token quarter
        if (ch < D && n0 + tq * 16 < a.Np) {
            const uint4 lo = *reinterpret_cast<const uint4*>(&vt[ch][tq * 16]), hi = *reinterpret_cast<const uint4*>(&vt[ch][tq * 16 + 8]);
            unsigned short* dst = a.vp + (g * D + ch) * a.Np + n0 + tq * 16;
            *reinterpret_cast<uint4*>(dst) = lo;
            *reinterpret_cast<uint4*>(dst + 8) = hi;
        }
    }
}

// Candidate groups along grid.y: doubled until `blocks` x groups reach `fill` blocks (enough to fill the chip when the source is small:
// weights) or every candidate has a group of its own; a thread then loops over the candidates of its group.
int64_t candidate_groups(int64_t blocks, int64_t fill, int64_t C) {
    int64_t by = 1;
    while (blocks * by < fill && by < C) by *= 2;
    return by;
}

template <typename T, int KIND>
int launch_pack(const PackArgs& a, hipStream_t st) {
    constexpr int EPT = Out<T>::EPT;
    const bool generic = getenv("ADALOG_PACK_GENERIC") != nullptr;           // read per call: the tests switch it
    if (a.sxk == 1) {
        const int64_t total = a.G * a.R * (a.Kp >> 2);
        int64_t gx = (total + 255) / 256;
        if (gx > 16384) gx = 16384;
        if (gx < 1) gx = 1;
        const int64_t gy = candidate_groups(gx, 2048, a.C);
        static const int use_tab = getenv("ADALOG_PACK_TAB") ? atoi(getenv("ADALOG_PACK_TAB")) : 1;
        if (KIND == KIND_UNIFORM && a.pr != 0 && use_tab && (a.Kp >> 2) >= 64 && a.C * TAB_ROWS * sizeof(float4) <= 64 * 1024 && !generic) {
            // per-row parameters (weight candidates): parameters staged in LDS per block, exact grid (no grid-stride loop)
            const size_t shm = (size_t)a.C * TAB_ROWS * sizeof(float4);
            if constexpr (sizeof(T) == 1) {
                // one-byte outputs, long aligned rows: 16 k per thread, 16-byte stores
                static const int use16 = getenv("ADALOG_PACK_TAB16") ? atoi(getenv("ADALOG_PACK_TAB16")) : 1;
                if (use16 && (a.K & 15) == 0 && (a.Kp & 15) == 0 && (a.Kp >> 4) >= 64 && (a.sxr & 3) == 0 && (a.sxg & 3) == 0 &&
                    ((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.out & 15) == 0) {
                    const int64_t bx16 = (a.G * a.R * (a.Kp >> 4) + 255) / 256;
                    if (bx16 < ((int64_t)1 << 31)) {
                        hipLaunchKernelGGL((k_pack_uniform_tab<T, 16>), dim3((unsigned)bx16, (unsigned)candidate_groups(bx16, 1024, a.C)),
                                           dim3(256), shm, st, a);
                        return 0;
                    }
                }
            }
            const int64_t bx = (total + 255) / 256;
            if (bx < ((int64_t)1 << 31)) {
                hipLaunchKernelGGL((k_pack_uniform_tab<T, 4>), dim3((unsigned)bx, (unsigned)candidate_groups(bx, 1024, a.C)), dim3(256), shm,
                                   st, a);
                return 0;
            }
        }
        if (KIND == KIND_UNIFORM && sizeof(T) == 1 && a.pr == 0 && (a.pg == 0 || a.G <= 65535) && !a.rowsum && a.C <= 2048 && !generic) {
            // per-tensor parameters: one grid over all groups; per-group (per-head) parameters: grid.z = groups
            int64_t fx = gx, fy = gy, fz = 1;
            if (a.pg != 0) {
                fz = a.G;
                fx = (a.R * (a.Kp >> 2) + 255) / 256;
                if (fx > 16384) fx = 16384;
                fy = candidate_groups(fx * fz, 2048, a.C);
            }
            hipLaunchKernelGGL((k_pack_uniform_i8_fast<std::is_same<T, fp8_t>::value>), dim3((unsigned)fx, (unsigned)fy, (unsigned)fz), dim3(256),
                               (size_t)a.C * sizeof(float4), st, a);
            return 0;
        }
        if constexpr (KIND == KIND_ADALOG) {
            // per-tensor scale and a table that fits in LDS; anything else (and ADALOG_PACK_GENERIC): k_pack, the exact path per element
            const size_t shm2 = (size_t)a.C * (sizeof(float4) + (size_t)(a.levels2 + 2) * sizeof(unsigned short));
            if (a.pg == 0 && !generic && shm2 <= 64 * 1024) {
                hipLaunchKernelGGL(k_pack_adalog_fast, dim3((unsigned)gx, (unsigned)gy), dim3(256), shm2, st, a);
                return 0;
            }
        } else {
            hipLaunchKernelGGL((k_pack_kfast<T, KIND>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, a);
            return 0;
        }
    }
    {
    const int64_t per_c = a.G * a.R * (a.Kp / EPT);
    int64_t gx = (per_c + 255) / 256;
    if (gx > 4096) gx = 4096;
    if (gx < 1) gx = 1;
    dim3 grid((unsigned)gx, (unsigned)a.C);
    const bool rfast = (a.sxr == 1 && a.sxk != 1);
    if (rfast)
        hipLaunchKernelGGL((k_pack<T, KIND, true>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((k_pack<T, KIND, false>), grid, dim3(256), 0, st, a);
    }
    return 0;
}

}  // namespace

// out dtype codes shared with gemm_score: 0 = int8, 1 = bf16, 2 = fp32
extern "C" int adalog_pack_uniform(const float* x, int64_t G, int64_t R, int64_t K, int64_t sxg, int64_t sxr, int64_t sxk,
                                   const float* scale, const float* zero_point, int64_t C, int64_t pc, int64_t gmod,
                                   int64_t pg, int64_t pr, int n_bits, int out_dtype, void* out, int64_t Kp,
                                   int32_t* rowsum, int c_inner, void* stream) {
    ADALOG_ARG_CHECK(x && scale && zero_point && out, "pack_uniform: null pointer");
    ADALOG_ARG_CHECK(G >= 1 && R >= 1 && K >= 1 && C >= 1 && C <= 65535 && gmod >= 1, "pack_uniform: bad sizes");
    ADALOG_ARG_CHECK(out_dtype != 3 || n_bits <= 4, "pack_uniform: fp8 output holds q - z exactly only for n_bits <= 4");
    {
        const int64_t row_bytes = Kp * ((out_dtype == 0 || out_dtype == 3) ? 1 : out_dtype == 1 ? 2 : 4);
        // 32-byte rows: int8 / fp8 operands of K <= 32 for the window kernel only (adalog_gemm_score checks its side)
        // rows of 16-byte slots, fp8 only: the candidate columns of the trimmed-K mixed kernel (adalog_gemm_mixed_ktrim: 208 bytes).  Every
        // pack kernel works on 4- or 16-element pieces of a row, so any such length packs; adalog_gemm_score checks what it can read
        ADALOG_ARG_CHECK(Kp >= K && (row_bytes % 64 == 0 || (row_bytes == 32 && (out_dtype == 0 || out_dtype == 3)) ||
                                     (row_bytes % 16 == 0 && out_dtype == 3)),
                         "pack_uniform: Kp must cover K and be a multiple of 64 bytes (128 for anything but the search kernels; fp8: of 16 bytes)");
    }
    ADALOG_ARG_CHECK(n_bits >= 2 && n_bits <= 7, "pack_uniform: n_bits must be in [2,7] (q - z must fit int8)");
    ADALOG_ARG_CHECK(!rowsum || C * G * R <= (int64_t)0x7fffffff, "pack_uniform: the row sums are indexed with 32 bits");
    hipStream_t st = (hipStream_t)stream;
    PackArgs a{};
    a.x = x; a.G = G; a.R = R; a.K = K; a.sxg = sxg; a.sxr = sxr; a.sxk = sxk;
    a.scale = scale; a.zp = zero_point; a.C = C; a.pc = pc; a.gmod = gmod; a.pg = pg; a.pr = pr;
    a.qmax = (float)((1 << n_bits) - 1); a.levels2 = 1 << n_bits; a.out = out; a.Kp = Kp; a.rowsum = rowsum; a.c_inner = c_inner;
    if (rowsum) {
        hipError_t e = hipMemsetAsync(rowsum, 0, sizeof(int32_t) * C * G * R, st);
        if (e != hipSuccess) { adalog_set_error("pack_uniform/memset", e); return (int)e; }
    }
    if (out_dtype == 0) launch_pack<int8_t, KIND_UNIFORM>(a, st);
    else if (out_dtype == 1) launch_pack<__hip_bfloat16, KIND_UNIFORM>(a, st);
    else if (out_dtype == 2) launch_pack<float, KIND_UNIFORM>(a, st);
    else if (out_dtype == 3) launch_pack<fp8_t, KIND_UNIFORM>(a, st);
    else { adalog_set_error_msg("pack_uniform: unknown out_dtype"); return -1; }
    ADALOG_LAUNCH_CHECK("adalog_pack_uniform");
    return 0;
}

// pre = 1: the operand is GELU(x) -- the activation function between fc1 and fc2 (reference timm Mlp / quant_layers/linear.py:770-796
// quant_forward) applied in the packer's loader, so that quant_forward of the MLP runs no separate GELU pass.  Per-tensor scale, unit
// stride along K only (the fast kernel); anything else is refused.
extern "C" int adalog_pack_adalog_bf16(const float* x, int64_t G, int64_t R, int64_t K, int64_t sxg, int64_t sxr,
                                       int64_t sxk, const float* scale, const float* qv, int64_t C, int64_t pc,
                                       int64_t gmod, int64_t pg, int n_bits, const float* mant37, const float* shift,
                                       int clamp_u, void* out, int64_t Kp, int c_inner, int pre, void* stream) {
    ADALOG_ARG_CHECK(pre == 0 || (pre == 1 && pg == 0 && sxk == 1 && !getenv("ADALOG_PACK_GENERIC")), "pack_adalog: the GELU prologue needs a per-tensor scale and unit K stride");
    ADALOG_ARG_CHECK(x && scale && qv && mant37 && out, "pack_adalog: null pointer");
    ADALOG_ARG_CHECK(G >= 1 && R >= 1 && K >= 1 && C >= 1 && C <= 65535 && gmod >= 1, "pack_adalog: bad sizes");
    // (rows of 16 elements: the fixed bf16 operand of the trimmed-K mixed kernel, adalog_gemm_mixed_ktrim)
    ADALOG_ARG_CHECK(Kp >= K && (Kp * 2) % 32 == 0, "pack_adalog: Kp must cover K and be a multiple of 16 elements");
    ADALOG_ARG_CHECK(n_bits >= 2 && n_bits <= 7, "pack_adalog: n_bits must be in [2,7] (numerators must fit bf16)");
    PackArgs a{};
    a.x = x; a.G = G; a.R = R; a.K = K; a.sxg = sxg; a.sxr = sxr; a.sxk = sxk;
    a.scale = scale; a.qv = qv; a.C = C; a.pc = pc; a.gmod = gmod; a.pg = pg; a.pr = 0;
    a.levels2 = 1 << n_bits; a.mant = mant37; a.shift = shift; a.clamp_u = clamp_u; a.out = out; a.Kp = Kp;
    a.c_inner = c_inner; a.pre = pre;
    ADALOG_ARG_CHECK(pre == 0 || (size_t)C * (sizeof(float4) + (size_t)(a.levels2 + 2) * sizeof(unsigned short)) <= 64 * 1024, "pack_adalog: the GELU prologue runs on the fast kernel only");
    launch_pack<__hip_bfloat16, KIND_ADALOG>(a, (hipStream_t)stream);
    ADALOG_LAUNCH_CHECK("adalog_pack_adalog_bf16");
    return 0;
}

extern "C" int adalog_pack_raw_f32(const float* x, int64_t G, int64_t R, int64_t K, int64_t sxg, int64_t sxr, int64_t sxk,
                                   void* out, int64_t Kp, void* stream) {
    ADALOG_ARG_CHECK(x && out && G >= 1 && R >= 1 && K >= 1, "pack_raw: bad arguments");
    ADALOG_ARG_CHECK(Kp >= K && Kp % 32 == 0, "pack_raw: Kp must cover K and be a multiple of 32 elements");
    PackArgs a{};
    a.x = x; a.G = G; a.R = R; a.K = K; a.sxg = sxg; a.sxr = sxr; a.sxk = sxk; a.C = 1; a.gmod = 1;
    a.out = out; a.Kp = Kp;
    launch_pack<float, KIND_RAW>(a, (hipStream_t)stream);
    ADALOG_LAUNCH_CHECK("adalog_pack_raw_f32");
    return 0;
}

// ---- three-term bf16 image of an UNQUANTISED fp32 operand (patch-embedding weight search: the input keeps 8 bits or more and is
// scored as it is, conv.py:226-255).  x = hi + mid + lo exactly (8 + 8 + 8 mantissa bits, each residual is exact in fp32), stored
// as [row][hi(0..Kt) | mid(0..Kt) | lo(0..Kt)]; against a candidate operand of exact small integers repeated three times along K
// the bf16 MFMA then accumulates the same fp32 products as the fp32 MFMA does, at 5x its rate.
namespace {
__device__ __forceinline__ unsigned bf16_rne(float v) {
    unsigned u = __float_as_uint(v);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}
__global__ __launch_bounds__(256) void k_pack_split3(const float* __restrict__ x, int64_t R, int64_t K, int64_t sxg, int64_t sxr, int64_t sxk,
                                                    uint16_t* __restrict__ out, int64_t Kt) {
    const int64_t g = blockIdx.z;
    for (int64_t row = blockIdx.y; row < R; row += gridDim.y) {
    uint16_t* o = out + (g * R + row) * 3 * Kt;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < Kt; k += (int64_t)gridDim.x * 256) {
        unsigned h = 0, m = 0, l = 0;
        if (k < K) {
            const float v = x[g * sxg + row * sxr + k * sxk];
            h = bf16_rne(v);
            const float r1 = v - __uint_as_float(h << 16);
            m = bf16_rne(r1);
            const float r2 = r1 - __uint_as_float(m << 16);
            l = bf16_rne(r2);
        }
        o[k] = (uint16_t)h; o[Kt + k] = (uint16_t)m; o[2 * Kt + k] = (uint16_t)l;
    }
    }
}
}  // namespace

extern "C" int adalog_pack_split3_bf16(const float* x, int64_t G, int64_t R, int64_t K, int64_t sxg, int64_t sxr, int64_t sxk,
                                       void* out, int64_t Kt, void* stream) {
    ADALOG_ARG_CHECK(x && out && G >= 1 && R >= 1 && K >= 1, "pack_split3: bad arguments");
    ADALOG_ARG_CHECK(Kt >= K && Kt % 32 == 0, "pack_split3: Kt must cover K and be a multiple of 32 elements");
    ADALOG_ARG_CHECK(G < 65536, "pack_split3: too many groups for one launch");
    const unsigned bx = (unsigned)((Kt + 255) / 256);
    hipLaunchKernelGGL(k_pack_split3, dim3(bx, (unsigned)(R < 65535 ? R : 65535), (unsigned)G), dim3(256), 0, (hipStream_t)stream, x, R, K, sxg, sxr, sxk,
                       (uint16_t*)out, Kt);
    ADALOG_LAUNCH_CHECK("adalog_pack_split3_bf16");
    return 0;
}

// ---- the three softmax packs: one launcher

namespace {

struct SoftmaxPackForm {
    const char* name;        // prefix of the error messages
    const char* entry;       // C symbol, for a failed launch
    const char* kernel;      // what adalog_note_kernel records
    int S_lo, S_hi;          // rows of S_lo <= S <= Kp <= S_hi scores
    bool bias;               // Swin's form: table and index required, `count` counts groups of S rows
    // Empty input (count == 0) returns 0 BEFORE the argument checks (null pointers pass), and a negative count is refused with the
    // null-pointer message.  false: the arguments are checked first, and a count outside [0, 2^31) has a message of its own.  The
    // entry points have differed in this since they were written; kept as it is.
    bool empty_first;
};

template <bool BIAS, int NS, int ROWS>
void softmax_pack_launch(const SoftmaxPackArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((k_softmax_adalog_pack_t<BIAS, NS, ROWS>), dim3((unsigned)((a.rows + 4 * ROWS - 1) / (4 * ROWS))), dim3(256), 0, st, a);
}

// checks in the order the entry points have always made them, then the kernel for the form and the row length
int softmax_pack(const SoftmaxPackForm& f, const float* x, int64_t count, int S, float mul, const float* scale, const float* qv, int n_bits,
                 const float* mant37, void* out, int64_t Kp, const float* table, const int64_t* index, const float* mask, int H, int nW,
                 void* stream) {
    if (f.empty_first && count == 0) return 0;
    char s_range[64];
    snprintf(s_range, sizeof(s_range), "%d <= S <= Kp <= %d, Kp a multiple of 32", f.S_lo, f.S_hi);
    const char* what =
        !(x && scale && qv && mant37 && out && (!f.bias || (table && index)) && (!f.empty_first || count > 0)) ? "null pointer"
        : !(S >= f.S_lo && S <= f.S_hi && Kp >= S && Kp <= f.S_hi && (Kp * 2) % 64 == 0) ? s_range
        : !(H >= 1 && count % H == 0 && (!mask || nW >= 1)) ? "G must be a multiple of H, nW >= 1 with a mask"
        : !(n_bits >= 2 && n_bits <= 7) ? "n_bits must be in [2,7]"
        : !(f.empty_first || (count >= 0 && count <= (int64_t)0x7fffffff)) ? "0 <= rows < 2^31"
        : nullptr;
    if (what) {
        char msg[160];
        snprintf(msg, sizeof(msg), "%s: %s", f.name, what);
        adalog_set_error_msg(msg);
        return -1;
    }
    if (count == 0) return 0;
    const SoftmaxPackArgs a{x, f.bias ? count * S : count, S, mul, scale, qv, mant37, 1 << n_bits, reinterpret_cast<unsigned short*>(out), Kp,
                            table, index, mask, H, mask ? nW : 1};
    adalog_note_kernel(f.kernel);
    hipStream_t st = (hipStream_t)stream;
    if (f.bias) softmax_pack_launch<true, 4, SM_ROWS>(a, st);
    else if (S <= 256) softmax_pack_launch<false, 4, SM_ROWS>(a, st);
    else if (S <= 512) softmax_pack_launch<false, 8, 2>(a, st);
    else softmax_pack_launch<false, 16, 1>(a, st);
    ADALOG_LAUNCH_CHECK(f.entry);
    return 0;
}

}  // namespace

// (x * mul).softmax(-1) quantised by the post-softmax AdaLog quantiser (per-tensor scale, log base 2^(-q/37), u clamped to
// [1e-15, 1]: reference quant_layers/matmul.py:337-343 with the searched q) straight into the bf16 operand image [rows][Kp] of
// the softmax . v product.  x: fp32 [rows][S] contiguous, S <= 256; Kp: a multiple of 32 elements covering S, <= 256.
extern "C" int adalog_softmax_adalog_pack_bf16(const float* x, int64_t rows, int S, float mul, const float* scale, const float* qv,
                                               int n_bits, const float* mant37, void* out, int64_t Kp, void* stream) {
    static const SoftmaxPackForm f{"softmax_adalog_pack", "adalog_softmax_adalog_pack_bf16", "k_softmax_adalog_pack", 1, 256, false, true};
    return softmax_pack(f, x, rows, S, mul, scale, qv, n_bits, mant37, out, Kp, nullptr, nullptr, nullptr, 1, 1, stream);
}

// The same for rows of 257 <= S <= 1024 scores (a ViT / DeiT at 384 px: 577 tokens): 8 slots per lane up to 512, 16 up to 1024, which is
// as far as ATen's per-warp softmax -- the arithmetic this kernel restates -- goes.  Kp: a multiple of 32 elements covering S, <= 1024.
extern "C" int adalog_softmax_adalog_pack_long_bf16(const float* x, int64_t rows, int S, float mul, const float* scale, const float* qv,
                                                    int n_bits, const float* mant37, void* out, int64_t Kp, void* stream) {
    static const SoftmaxPackForm f{"softmax_adalog_pack_long", "adalog_softmax_adalog_pack_long_bf16", "k_softmax_adalog_pack_long", 257,
                                   1024, false, false};
    return softmax_pack(f, x, rows, S, mul, scale, qv, n_bits, mant37, out, Kp, nullptr, nullptr, nullptr, 1, 1, stream);
}

// Swin's window attention: ((x + relative-position bias) + shift mask).softmax(-1) through the same quantiser into the same operand
// image.  x: fp32 [G][S][S] contiguous (G = windows * H); table fp32 [(2 Wh - 1)(2 Ww - 1)][H] contiguous; index int64 [S][S] (entries
// index the table's rows); mask fp32 [nW][S][S] or null, window w = (g / H) % nW.  The table is read on every call (no cached bias).
extern "C" int adalog_softmax_bias_adalog_pack_bf16(const float* x, int64_t G, int S, int H, const float* table, const int64_t* index,
                                                    const float* mask, int nW, const float* scale, const float* qv, int n_bits,
                                                    const float* mant37, void* out, int64_t Kp, void* stream) {
    static const SoftmaxPackForm f{"softmax_bias_adalog_pack", "adalog_softmax_bias_adalog_pack_bf16", "k_softmax_bias_adalog_pack", 1, 256,
                                   true, true};
    return softmax_pack(f, x, G, S, 1.0f, scale, qv, n_bits, mant37, out, Kp, table, index, mask, H, nW, stream);
}

// The three operand packs of an attention block's quant_forward in one launch per 65535 images (k_attn_split_pack): qkv fp32
// [B][N][3][H][D] (contiguous, 16-byte aligned), D in {16, 32, 48, 64}; (scale, zero point) of the three uniform quantisers per head
// (pg = 1: [H]) or per tensor (pg = 0); qp, kp int8 [B*H][N][128]; vp bf16 [B*H][D][Np], Np a multiple of 64 covering N.  q_mul != 1:
// q is multiplied by it (fp32) before its quantiser.  Images beyond grid z's 65535 go in further launches (Swin: B = windows).
extern "C" int adalog_attn_split_pack(const float* qkv, int B, int N, int H, int D, float q_mul, const float* q_scale, const float* q_zp,
                                      int q_bits, const float* k_scale, const float* k_zp, int k_bits, const float* v_scale,
                                      const float* v_zp, int v_bits, int pg, void* qp, void* kp, void* vp, int64_t Np, void* stream) {
    if (B == 0 || N == 0) return 0;
    ADALOG_ARG_CHECK(qkv && q_scale && q_zp && k_scale && k_zp && v_scale && v_zp && qp && kp && vp, "attn_split_pack: null pointer");
    ADALOG_ARG_CHECK(B >= 1 && N >= 1 && H >= 1 && H <= 65535 && Np >= N && Np % 64 == 0, "attn_split_pack: bad sizes (Np: a multiple of 64 covering N)");
    ADALOG_ARG_CHECK(D >= 16 && D <= 64 && D % 16 == 0, "attn_split_pack: head dimension must be 16, 32, 48 or 64");
    ADALOG_ARG_CHECK(q_bits >= 2 && q_bits <= 7 && k_bits >= 2 && k_bits <= 7 && v_bits >= 2 && v_bits <= 7, "attn_split_pack: n_bits must be in [2,7]");
    ADALOG_ARG_CHECK(((((uintptr_t)qkv) | ((uintptr_t)qp) | ((uintptr_t)kp) | ((uintptr_t)vp)) & 15) == 0, "attn_split_pack: 16-byte aligned buffers");
    const bool qmul = q_mul != 1.0f;
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        const int64_t gb = (int64_t)b0 * H;
        AttnSplitArgs a{qkv + (int64_t)b0 * N * 3 * H * D, nb, N, H, q_scale, q_zp, k_scale, k_zp, v_scale, v_zp, pg ? 1 : 0,
                        (float)((1 << q_bits) - 1), (float)((1 << k_bits) - 1), (float)((1 << v_bits) - 1),
                        reinterpret_cast<int8_t*>(qp) + gb * N * 128, reinterpret_cast<int8_t*>(kp) + gb * N * 128,
                        reinterpret_cast<unsigned short*>(vp) + gb * D * Np, Np, q_mul};
        const dim3 grid((unsigned)(Np / 64), (unsigned)H, (unsigned)nb);
        adalog_dispatch<1, 2, 3, 4>(D / 16, [&](auto qd) {
            return adalog_dispatch<true, false>(qmul, [&](auto qm) {
                return adalog_launch<k_attn_split_pack<decltype(qd)::value, decltype(qm)::value>>("k_attn_split_pack", 0, grid, 256, 0,
                                                                                                  (hipStream_t)stream, a);
            });
        });
        ADALOG_LAUNCH_CHECK("adalog_attn_split_pack");
    }
    return 0;
}
