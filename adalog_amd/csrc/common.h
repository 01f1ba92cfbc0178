// Shared device/host helpers for the AdaLog MI355X (gfx950) kernels.
// Compiled with hipcc --offload-arch=gfx950 -ffp-contract=off: every fp32 step below must round exactly
// like the reference's ATen CPU op (IEEE divide, round-half-even, no FMA contraction).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <type_traits>
#include "../../include/adalog_hip.h"   // the public C ABI: every definition is compiled against its declaration

#define ADALOG_R 37            // AdaLog fixed denominator r (reference quantizers/logarithm.py:71)

extern "C" void adalog_set_error(const char* where, hipError_t e);
extern "C" void adalog_set_error_msg(const char* msg);
extern "C" void adalog_note_kernel(const char* name);
extern "C" unsigned int* adalog_ticket_slot(void);      // brecq.hip: a zeroed device word for "last block finishes" kernels
extern "C" unsigned int* adalog_ticket_slots(int n);    // ... n <= 64 consecutive zeroed words
extern "C" unsigned int* adalog_ticket_slots_on(int n, void* stream);   // ... from the sub-ring of that stream

#define ADALOG_LAUNCH_CHECK(name)                                   \
    do {                                                            \
        hipError_t e__ = hipGetLastError();                         \
        if (e__ != hipSuccess) { adalog_set_error(name, e__); return (int)e__; } \
    } while (0)

#define ADALOG_ARG_CHECK(cond, msg)                                 \
    do { if (!(cond)) { adalog_set_error_msg(msg); return -1; } } while (0)

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// Raise a kernel's dynamic-LDS limit once PER DEVICE (the attribute belongs to the function's code object on one device: a
// per-process "done" flag would leave the second device of a process without it).  ``done_mask``: a static per call site, one bit
// per device ordinal.  Returns the error of hipFuncSetAttribute so that the caller fails instead of launching with 64 KiB.
static inline hipError_t adalog_max_lds(const void* fn, int bytes, unsigned long long* done_mask) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (*done_mask & bit) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) *done_mask |= bit;
    return e;
}

// ... for kernel instantiation K, to max_lds bytes.  K is a template argument, so the once-per-device state is one per instantiation.
// 0, or the HIP error (recorded).
template <auto K>
static inline int adalog_lds_limit(int max_lds) {
    static unsigned long long attr_dev = 0;
    const hipError_t e = adalog_max_lds(reinterpret_cast<const void*>(K), max_lds, &attr_dev);
    if (e != hipSuccess) { adalog_set_error("hipFuncSetAttribute", e); return (int)e; }
    return 0;
}

// Launch of kernel instantiation K: raise its dynamic-LDS limit (max_lds = 0: the default limit is enough), note the label for
// adalog_last_kernel (a string literal: the pointer is kept), launch.  0, or the HIP error of the limit call.
template <auto K, class... Args>
static inline int adalog_launch(const char* label, int max_lds, dim3 grid, int threads, size_t shm, hipStream_t st, const Args&... args) {
    if (max_lds > 0)
        if (const int e = adalog_lds_limit<K>(max_lds)) return e;
    adalog_note_kernel(label);
    hipLaunchKernelGGL(K, grid, dim3((unsigned)threads), shm, st, args...);
    return 0;
}

// A run-time value from a fixed list as a compile-time constant: f(std::integral_constant<.., V>{}) for the V that equals v; the LAST
// value of the list is taken when none does (the closing `else` of an if-ladder).  Nested calls enumerate a kernel's instantiations.
template <auto V0, auto... Vs, class T, class F>
static inline int adalog_dispatch(T v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<decltype(V0), V0>{});
    else return v == V0 ? f(std::integral_constant<decltype(V0), V0>{}) : adalog_dispatch<Vs...>(v, f);
}

// compute units of the CURRENT device (cached per device ordinal, not per process)
static inline int adalog_device_cus() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    int& c = cus[dev & 63];
    if (c == 0) {
        hipDeviceProp_t pr;
        c = (hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
    }
    return c;
}

// ---------------------------------------------------------------------------------------------- device math
// asymmetric uniform bin: clamp(rne(x / s) + z, 0, qmax)       (uniform.py:29-35; z already rounded)
// ... and the code in front of the clamp, rne(x / s) + z: what the code histogram (report.hip) sorts into below / code / above
__device__ __forceinline__ float uni_code(float x, float s, float z) {
    float xi = rintf(x / s);
    return xi + z;
}
__device__ __forceinline__ float uni_bin(float x, float s, float z, float qmax) {
    return fminf(fmaxf(uni_code(x, s, z), 0.0f), qmax);
}

// k = rne( (-log2(u)) * 37 / q ) with u a positive float, evaluated so that it equals the fp32 pipeline
//   L = fl32(log2 u) correctly rounded;  t = fl32(fl32(-L * 37) / q);  k = rne(t)
// (logarithm.py:94 with a correctly-rounded log2; torch's SLEEF log2 differs from correct rounding on <1e-3 of
// inputs by one ulp, which moves k only for t within one ulp of a tie: ~1e-9 of elements).
// Fast path: hardware v_log_f32 (1 ulp) unless t lands within 1e-3 of a tie; then the exact path in fp64.
__device__ __forceinline__ float adalog_k(float u, float qf) {
    float lf = __log2f(u);
    float t = (-lf) * 37.0f / qf;
    float k = rintf(t);
    float fr = fabsf(t - k);
    if (__builtin_expect(fr > 0.499f || !(t < 3.0e38f), 0)) {
        float le = (float)log2((double)u);
        t = (-le) * 37.0f / qf;
        k = rintf(t);
    }
    return k;
}

// pk.byte[pos] = rne(tc) as a two's-complement int8 (|tc| <= 127; pos a compile-time constant after inlining): ONE SDWA add of
// 1.5 * 2^23 rounds to nearest-even (the sum's ulp is 1), and the low byte of the sum's bit pattern IS the integer -- rounding,
// conversion and the byte insert of a generated int8 MFMA operand in one VALU instruction (round 5; gram.hip, gram_act.hip).
__device__ __forceinline__ int sdwa_rne_byte(int pk, float tc, float magic /* 12582912.0f */, int pos) {
    if (pos == 0) asm("v_add_f32_sdwa %0, %1, %2 dst_sel:BYTE_0 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(pk) : "v"(tc), "v"(magic));
    else if (pos == 1) asm("v_add_f32_sdwa %0, %1, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(pk) : "v"(tc), "v"(magic));
    else if (pos == 2) asm("v_add_f32_sdwa %0, %1, %2 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(pk) : "v"(tc), "v"(magic));
    else asm("v_add_f32_sdwa %0, %1, %2 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(pk) : "v"(tc), "v"(magic));
    return pk;
}

// ---- QDrop (activation dropping inside a BRECQ iteration): element e of a quantiser's output keeps its fake-quantised value when
// u_e < p and passes through unquantised otherwise.  u_e comes from Philox4x32-10 (Salmon et al., SC'11), a counter-based generator:
// no mask is stored, the backward pass of an iteration regenerates the mask of its forward.
//   key     = (seed_lo, seed_hi)
//   counter = (e >> 2 low word, e >> 2 high word, iteration, stream)          -- one Philox block per four consecutive elements
//   u_e     = float(word[e & 3] >> 8) * 2^-24                                 -- p = 1 keeps everything, p = 0 nothing
// seed and iteration are read from device memory (state = {seed_lo, seed_hi, iteration}): a captured HIP graph draws a new mask
// on every replay.  ``stream`` tells the quantisers of a block apart.
struct DropArgs {
    const uint32_t* state;
    uint32_t stream;
    float p;
};

__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// the Philox block of elements 4 * blk .. 4 * blk + 3 of this quantiser in this iteration
__device__ __forceinline__ uint4 drop_words(const DropArgs& d, int64_t blk) {
    return philox4x32_10((uint32_t)blk, (uint32_t)((uint64_t)blk >> 32), d.state[2], d.stream, d.state[0], d.state[1]);
}
__device__ __forceinline__ bool drop_keep(uint32_t word, float p) { return (float)(word >> 8) * 5.9604644775390625e-8f < p; }
// ... of the single element e (the scalar paths: rows that are no multiple of four, unaligned tensors)
__device__ __forceinline__ bool drop_keep_at(const DropArgs& d, int64_t e) {
    const uint4 w = drop_words(d, e >> 2);
    const int j = (int)(e & 3);
    return drop_keep(j == 0 ? w.x : (j == 1 ? w.y : (j == 2 ? w.z : w.w)), d.p);
}

// ---- fast forms used by the operand-packing kernels (hundreds of millions of elements per scoring call).
// Both evaluate with a reciprocal multiply first and fall back to the exact IEEE sequence above only when the result
// lands within 1e-3 of a rounding tie, so they return EXACTLY the same integer as the exact forms (the reciprocal path
// is accurate to ~3 ulp, i.e. < 1e-4 absolute at the magnitudes that survive the clamp).
__device__ __forceinline__ float uni_bin_fast(float x, float s, float inv_s, float z, float qmax) {
    float t = x * inv_s;
    float k = rintf(t);
    if (__builtin_expect(fabsf(t - k) > 0.499f && fabsf(t) < 4096.0f, 0)) k = rintf(x / s);
    return fminf(fmaxf(k + z, 0.0f), qmax);
}

// xs = x (+ shift); returns k = rne(-log2(clamp(xs/s)) * 37 / q) exactly as adalog_k(clamp(xs / s), q)
__device__ __forceinline__ float adalog_k_fast(float xs, float s, float inv_s, float qf, float rq37, bool clamp_u) {
    float u = xs * inv_s;
    if (clamp_u) u = fminf(fmaxf(u, 1e-15f), 1.0f);
    float t = -__log2f(u) * rq37;
    float k = rintf(t);
    if (__builtin_expect(fabsf(t - k) > 0.499f || !(t < 3.0e38f), 0)) {
        float ue = xs / s;
        if (clamp_u) ue = fminf(fmaxf(ue, 1e-15f), 1.0f);
        float le = (float)log2((double)ue);
        t = (-le) * 37.0f / qf;
        k = rintf(t);
    }
    return k;
}

// The bin of the AdaLog / ShiftAdaLog fake-quantiser, shared by k_adalog (fakequant.hip: its ``bins`` output and its LUT index) and
// the bin histogram (report.hip): v -> GELU(v) when ``pre`` (ATen's fp32 erf expression), + shift, k = adalog_k_fast(.., clamp_u).
// Returns k clamped to [0, levels2 - 1]; keep = k < levels2 (otherwise the element takes the masked code 255 and the value 0).
__device__ __forceinline__ float adalog_fq_bin(float v, float s, float inv_s, float qf, float rq37, bool has_shift, float sh, int pre,
                                               int levels2, bool& keep) {
    if (pre) v = (v * 0.5f) * (1.0f + erff(v * 0.70710678118654752440f));   // GELU (ATen's fp32 expression): fc2 reads fc1's output
    const float xs = has_shift ? v + sh : v;
    const float k = adalog_k_fast(xs, s, inv_s, qf, rq37, true);
    keep = k < (float)levels2;
    return fminf(fmaxf(k, 0.0f), (float)(levels2 - 1));
}
