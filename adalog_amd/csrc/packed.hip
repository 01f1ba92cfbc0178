// Packed low-bit weight codes: the storage format "adalog-packed-v1" of a calibrated checkpoint (utils/packed.py).
//
// A weight viewed as [R][K] becomes uint32 [R][B * ceil(K / 32)]: every row is cut into groups of 32 consecutive codes and a group
// occupies exactly B words.  Code i of a group (0 <= i < 32) sits at bits [i B, (i + 1) B) of the group's little-endian bit stream
// (stream bit j = bit j % 32 of word j / 32); codes beyond K are 0.  The code is the one the fake-quantiser and the operand packers
// compute, q = clamp(rne(w / s) + rne(z), 0, 2^B - 1) (uni_bin of common.h, -ffp-contract=off), so that the weight rebuilt from the
// codes, (q - rne(z)) * s, quantises to the same q again: every quant_forward route computes what it computed from the fp32 weight.
//
// Both kernels stream: eight lanes share a group, each owns four consecutive codes.  A wavefront then reads (pack) or writes (unpack)
// 1 KiB of contiguous fp32 per instruction -- one group per lane would touch 64 different 128-byte lines per instruction -- and no
// output word is shared between groups, so nothing is atomic.  The eight partial bit fields of a group are OR-ed with three
// butterfly shuffles per word and lane l < B stores word l.
#include "common.h"
#include <hip/hip_bf16.h>

namespace {

constexpr int LANES = 8;          // lanes per group of 32 codes
constexpr int CPL = 32 / LANES;   // codes per lane

inline int grid_for_threads(int64_t threads) {
    int64_t b = (threads + 255) / 256;
    if (b < 1) b = 1;
    if (b > 16384) b = 16384;     // grid-stride the rest
    return (int)b;
}

template <int B, bool VEC>
__global__ __launch_bounds__(256) void k_pack_codes(const float* __restrict__ w, int64_t R, int64_t K, int64_t ldw,
                                                    const float* __restrict__ scale, const float* __restrict__ zp, int per_row,
                                                    uint32_t* __restrict__ out) {
    const int64_t gpr = (K + 31) >> 5;                       // groups per row
    const int64_t ngroups = R * gpr;
    const int l = threadIdx.x & (LANES - 1);
    const float qmax = (float)((1 << B) - 1);
    const int p = l * CPL * B, w0 = p >> 5, sh = p & 31;    // this lane's bit field inside the group's stream
    // (the loop bound is uniform over the eight lanes of a group: the shuffles below only cross lanes of one group)
    for (int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LANES; g < ngroups;
         g += ((int64_t)gridDim.x * blockDim.x) / LANES) {
        const int64_t row = g / gpr, gi = g - row * gpr;
        const int64_t pi = per_row ? row : 0;
        const float s = scale[pi], z = rintf(zp[pi]);
        const int64_t k0 = gi * 32 + l * CPL;
        const float* wr = w + row * ldw;
        float x[CPL] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (VEC && k0 + CPL <= K) {
            const float4 v = *reinterpret_cast<const float4*>(wr + k0);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
#pragma unroll
            for (int e = 0; e < CPL; ++e)
                if (k0 + e < K) x[e] = wr[k0 + e];
        }
        uint32_t v = 0;
#pragma unroll
        for (int e = 0; e < CPL; ++e)
            if (k0 + e < K) v |= ((uint32_t)(int)uni_bin(x[e], s, z, qmax) & (uint32_t)((1 << B) - 1)) << (e * B);
        const uint64_t t = (uint64_t)v << sh;
        const uint32_t lo = (uint32_t)t, hi = (uint32_t)(t >> 32);
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < B; ++j) {
            uint32_t m = (w0 == j ? lo : 0u) | (w0 + 1 == j ? hi : 0u);
            m |= __shfl_xor(m, 1);
            m |= __shfl_xor(m, 2);
            m |= __shfl_xor(m, 4);
            if (l == j) mine = m;
        }
        if (l < B) out[(row * gpr + gi) * B + l] = mine;
    }
}

template <typename T> __device__ __forceinline__ T to_out(float v);
template <> __device__ __forceinline__ float to_out<float>(float v) { return v; }
template <> __device__ __forceinline__ int8_t to_out<int8_t>(float v) { return (int8_t)(int)v; }
template <> __device__ __forceinline__ __hip_bfloat16 to_out<__hip_bfloat16>(float v) { return __float2bfloat16(v); }

// IMAGE = false: out = (q - rne(z)) * s, columns [0, K) of rows of ldo elements, the rest untouched.
// IMAGE = true:  out = q - rne(z) as T (the operand image of adalog_pack_uniform), columns [K, ldo) written as zero.
template <typename T, int B, bool IMAGE, bool VEC>
__global__ __launch_bounds__(256) void k_unpack_codes(const uint32_t* __restrict__ in, int64_t R, int64_t K,
                                                      const float* __restrict__ scale, const float* __restrict__ zp, int per_row,
                                                      T* __restrict__ out, int64_t ldo) {
    const int64_t gpr = (K + 31) >> 5;                       // groups per row that hold codes
    const int64_t limit = IMAGE ? ldo : K;                   // columns written per row
    const int64_t gpo = (limit + 31) >> 5;
    const int64_t ngroups = R * gpo;
    const int l = threadIdx.x & (LANES - 1);
    const int p = l * CPL * B, w0 = p >> 5, sh = p & 31;
    const float qmax = (float)((1 << B) - 1);
    for (int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LANES; g < ngroups;
         g += ((int64_t)gridDim.x * blockDim.x) / LANES) {
        const int64_t row = g / gpo, gi = g - row * gpo;
        const int64_t k0 = gi * 32 + l * CPL;
        if (k0 >= limit) continue;
        const int64_t pi = per_row ? row : 0;
        const float s = scale[pi], z = rintf(zp[pi]);
        uint32_t v = 0;
        if (k0 < K) {                                        // (then gi < gpr: the group exists in the packed row)
            const uint32_t* gp = in + (row * gpr + gi) * B;
            uint64_t t = gp[w0];
            if (sh + CPL * B > 32) t |= (uint64_t)gp[w0 + 1] << 32;     // (the field ends inside the group: w0 + 1 < B)
            v = (uint32_t)(t >> sh);
        }
        alignas(16) T vals[CPL];
#pragma unroll
        for (int e = 0; e < CPL; ++e) {
            const float q = (float)((v >> (e * B)) & (uint32_t)((1 << B) - 1));
            float c = q - z;
            // the image through the packers' own clamp (operand.hip: med3(k, -z, qmax - z)): c is inside it, so this changes no value, but
            // the sign of a zero is then the one adalog_pack_uniform writes for the rebuilt weight (a bound can be -0)
            if (IMAGE) c = __builtin_amdgcn_fmed3f(c, -z, qmax - z);
            vals[e] = to_out<T>(k0 + e < K ? (IMAGE ? c : c * s) : 0.0f);
        }
        T* op = out + row * ldo + k0;
        if (VEC && k0 + CPL <= limit) {
            if constexpr (sizeof(T) == 4) *reinterpret_cast<uint4*>(op) = *reinterpret_cast<const uint4*>(vals);
            else if constexpr (sizeof(T) == 2) *reinterpret_cast<uint2*>(op) = *reinterpret_cast<const uint2*>(vals);
            else *reinterpret_cast<uint32_t*>(op) = *reinterpret_cast<const uint32_t*>(vals);
        } else {
#pragma unroll
            for (int e = 0; e < CPL; ++e)
                if (k0 + e < limit) op[e] = vals[e];
        }
    }
}

template <typename T, bool IMAGE>
int launch_unpack(const uint32_t* in, int64_t R, int64_t K, const float* scale, const float* zp, int per_row, int n_bits, T* out,
                  int64_t ldo, hipStream_t st) {
    const int64_t limit = IMAGE ? ldo : K;
    const int64_t threads = R * ((limit + 31) >> 5) * LANES;
    const bool vec = (ldo % CPL == 0) && ((uintptr_t)out % (CPL * sizeof(T)) == 0);
    const dim3 grid((unsigned)grid_for_threads(threads));
    return adalog_dispatch<2, 3, 4, 5, 6, 7, 8>(n_bits, [&](auto b) {
        constexpr int B = decltype(b)::value;
        if (vec) return adalog_launch<k_unpack_codes<T, B, IMAGE, true>>("k_unpack_codes", 0, grid, 256, 0, st, in, R, K, scale, zp, per_row, out, ldo);
        return adalog_launch<k_unpack_codes<T, B, IMAGE, false>>("k_unpack_codes", 0, grid, 256, 0, st, in, R, K, scale, zp, per_row, out, ldo);
    });
}

// R * ceil(K / 32) groups of eight lanes must stay far inside int64 and the packed row inside the int the size query returns
inline bool sizes_ok(int64_t R, int64_t K) { return R >= 1 && K >= 1 && K <= ((int64_t)1 << 27) && R <= ((int64_t)1 << 31); }

}  // namespace

extern "C" int64_t adalog_packed_row_words(int64_t K, int n_bits) {
    if (K < 1 || K > ((int64_t)1 << 27) || n_bits < 2 || n_bits > 8) return -1;
    return (int64_t)n_bits * ((K + 31) >> 5);
}

extern "C" int adalog_pack_codes_f32(const float* w, int64_t R, int64_t K, int64_t ldw, const float* scale, const float* zero_point,
                                     int per_row, int n_bits, uint32_t* out, void* stream) {
    ADALOG_ARG_CHECK(w && scale && zero_point && out, "pack_codes: null pointer");
    ADALOG_ARG_CHECK(n_bits >= 2 && n_bits <= 8, "pack_codes: n_bits must be in [2,8]");
    ADALOG_ARG_CHECK(sizes_ok(R, K) && ldw >= K, "pack_codes: bad sizes (R >= 1, 1 <= K <= 2^27, ldw >= K)");
    ADALOG_ARG_CHECK(per_row == 0 || per_row == 1, "pack_codes: per_row must be 0 or 1");
    hipStream_t st = (hipStream_t)stream;
    const int64_t threads = R * ((K + 31) >> 5) * LANES;
    const bool vec = (ldw % CPL == 0) && ((uintptr_t)w % 16 == 0);
    const dim3 grid((unsigned)grid_for_threads(threads));
    const int rc = adalog_dispatch<2, 3, 4, 5, 6, 7, 8>(n_bits, [&](auto b) {
        constexpr int B = decltype(b)::value;
        if (vec) return adalog_launch<k_pack_codes<B, true>>("k_pack_codes", 0, grid, 256, 0, st, w, R, K, ldw, scale, zero_point, per_row, out);
        return adalog_launch<k_pack_codes<B, false>>("k_pack_codes", 0, grid, 256, 0, st, w, R, K, ldw, scale, zero_point, per_row, out);
    });
    if (rc) return rc;
    ADALOG_LAUNCH_CHECK("adalog_pack_codes_f32");
    return 0;
}

extern "C" int adalog_unpack_codes(const uint32_t* in, int64_t R, int64_t K, const float* scale, const float* zero_point, int per_row,
                                   int n_bits, int out_dtype, void* out, int64_t ldo, void* stream) {
    ADALOG_ARG_CHECK(in && scale && zero_point && out, "unpack_codes: null pointer");
    ADALOG_ARG_CHECK(n_bits >= 2 && n_bits <= 8, "unpack_codes: n_bits must be in [2,8]");
    ADALOG_ARG_CHECK(out_dtype >= 0 && out_dtype <= 2, "unpack_codes: out_dtype must be 0 (int8), 1 (bf16) or 2 (fp32)");
    ADALOG_ARG_CHECK(out_dtype != 0 || n_bits <= 7, "unpack_codes: the int8 image needs n_bits <= 7 (q - z must fit int8)");
    ADALOG_ARG_CHECK(sizes_ok(R, K) && ldo >= K && ldo <= ((int64_t)1 << 28), "unpack_codes: bad sizes (R >= 1, 1 <= K <= 2^27, ldo >= K)");
    ADALOG_ARG_CHECK(per_row == 0 || per_row == 1, "unpack_codes: per_row must be 0 or 1");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (out_dtype == 0) rc = launch_unpack<int8_t, true>(in, R, K, scale, zero_point, per_row, n_bits, (int8_t*)out, ldo, st);
    else if (out_dtype == 1) rc = launch_unpack<__hip_bfloat16, true>(in, R, K, scale, zero_point, per_row, n_bits, (__hip_bfloat16*)out, ldo, st);
    else rc = launch_unpack<float, false>(in, R, K, scale, zero_point, per_row, n_bits, (float*)out, ldo, st);
    if (rc) return rc;
    ADALOG_LAUNCH_CHECK("adalog_unpack_codes");
    return 0;
}
