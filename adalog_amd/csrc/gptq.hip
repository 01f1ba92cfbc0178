// GPTQ column sweep (Frantar et al., ICLR 2023) of one layer's weight in ONE launch (utils/gptq.py; no counterpart in the reference).
//
// Specification, per row r of W [R][K] (rows never interact), with U fp64 upper triangular, H^-1 = U^T U:
//   run = double(W[r, :])
//   for j = 0 .. K-1:   c_j = clamp(uni_code(float(run_j), s, rne(z)), 0, 2^b - 1)        fp32, the function k_uniform_rows / pack_codes use
//                       q_j = (c_j - rne(z)) * s                                           fp32, as unpack_codes(F32) computes it
//                       e_j = (run_j - double(q_j)) / U[j][j]                              fp64
//                       run_k = run_k - e_j * U[j][k]   for k > j                          fp64: one multiply, one subtract
// Every element run_k therefore sees its updates in ascending j, each a separately rounded multiply and subtract: in IEEE arithmetic
// the recurrence has ONE result, and the kernel produces it bit for bit (tests/gptq_reference.py is its numpy restatement).
//
// Layout.  A wavefront owns RPW rows and keeps each running row in registers, column k at lane k % 64, slot k / 64 (NI = ceil(K / 64)
// slots; 64 fp64 slots per lane at K = 4096).  The sweep walks the row in blocks of 64 columns (a slot):
//   1. the block's own 64 steps run in order: the step's value is broadcast from its lane (v_readlane), every lane forms c, q and e
//      from the broadcast (wave-uniform work, no divergence), lane l keeps q, c and e of step l, lanes > l update their column of the
//      block.  The 64 values U[j][block] a step reads are prefetched PF steps ahead, so the dependent chain of a step is
//      broadcast -> quantise -> divide -> multiply, subtract.
//   2. the 64 errors then go to every later slot: run[slot] -= e_l * U[j0 + l][slot's column] for l = 0 .. 63 IN THIS ORDER.  For one
//      element that is the same sequence of operations as the column-by-column sweep applies (a later slot is not read before its own
//      block starts), so the result is the specification's; for the machine it is a loop of independent coalesced reads of U (a row
//      segment of 512 bytes per wave instruction, the same for every wave: L2 traffic) feeding NI - slot independent fp64 chains.
// The slots are register arrays, so every slot index is a compile-time constant: the loops over slots are unrolled over the template
// bound NI_MAX in groups of G slots, a group is entered through one wave-uniform branch per block, and a slot of an entered group
// that is already finished (or beyond K) is updated harmlessly from a clamped, in-bounds address -- it is never read again.
// No LDS, no barrier, no atomics, no inter-workgroup traffic; What and the codes leave through coalesced per-block vector stores.
//
// Act-order (adalog_gptq_sweep_perm_f32, k_gptq_sweep_perm).  Step j works on column perm[j] of W, U factors the PERMUTED Hessian,
// What and the codes are stored in natural order.  The layout above is indexed by the STEP: slot i, lane l holds step 64 i + l.  Only the
// two ends touch a column: the load of the running row reads w[r][perm[64 i + l]] and the per-block store writes q and c of step
// 64 i + l to column perm[64 i + l] -- perm is read coalesced (256 bytes per block), the 64 lanes of an instruction scatter inside ONE
// row of at most 16 KiB, which they cover completely by the end of the sweep.  No permuted copy of W and no un-permute pass exist.
// perm comes from the caller's device memory, so k_perm_check proves it a permutation before either kernel indexes with it.
#include "common.h"
#include <mutex>

#pragma clang fp contract(off)

namespace {

constexpr int PF = 4;     // steps a block's own U values are read ahead of their use

__device__ __forceinline__ double bcast(double v, int lane) {        // lane: wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// k_gptq_sweep and k_gptq_sweep_perm are ONE text, gptq_sweep.inc, compiled twice: the natural-order kernel sees exactly the
// source it had before act-order existed (the same instructions), the other one the gather and the scatter as well.
#define SWEEP_KERNEL k_gptq_sweep
#define SWEEP_PERM 0
#include "gptq_sweep.inc"
#undef SWEEP_KERNEL
#undef SWEEP_PERM
#define SWEEP_KERNEL k_gptq_sweep_perm
#define SWEEP_PERM 1
#include "gptq_sweep.inc"
#undef SWEEP_KERNEL
#undef SWEEP_PERM

// perm == nullptr: the natural-order kernel
template <int NI_MAX, int G, int RPW>
int launch_sweep(const float* w, int64_t R, int64_t K, int64_t ldw, const float* scale, const float* zp, int per_row, int n_bits,
                 const double* U, int64_t ldu, const int32_t* perm, float* what, uint8_t* codes, double* objective, hipStream_t st) {
    const int64_t waves = (R + RPW - 1) / RPW;
    const int wpb = waves >= 1024 ? 4 : 1;                           // few rows: one wave per workgroup spreads them over the CUs
    const dim3 grid((unsigned)((waves + wpb - 1) / wpb));
    const float qmax = (float)((1 << n_bits) - 1);
    if (perm)
        return adalog_launch<k_gptq_sweep_perm<NI_MAX, G, RPW>>("k_gptq_sweep_perm", 0, grid, 64 * wpb, 0, st, w, R, (int)K, ldw, scale, zp,
                                                                per_row, qmax, U, ldu, perm, what, codes, objective);
    return adalog_launch<k_gptq_sweep<NI_MAX, G, RPW>>("k_gptq_sweep", 0, grid, 64 * wpb, 0, st, w, R, (int)K, ldw, scale, zp, per_row,
                                                       qmax, U, ldu, what, codes, objective);
}

// the slot-count instantiation of a shape, shared by the two entry points
int sweep(const float* w, int64_t R, int64_t K, int64_t ldw, const float* scale, const float* zero_point, int per_row, int n_bits,
          const double* U, int64_t ldu, const int32_t* perm, float* what, uint8_t* codes, double* objective, hipStream_t st) {
    const int ni = (int)((K + 63) >> 6);
    const bool two = R > 2048;                                       // two rows per wave halve the reads of U once the SIMDs are full
#define SWEEP(NI_MAX, G, RPW) launch_sweep<NI_MAX, G, RPW>(w, R, K, ldw, scale, zero_point, per_row, n_bits, U, ldu, perm, what, codes, objective, st)
    if (ni <= 4) return two ? SWEEP(4, 1, 2) : SWEEP(4, 1, 1);
    if (ni <= 8) return two ? SWEEP(8, 2, 2) : SWEEP(8, 2, 1);
    if (ni <= 16) return two ? SWEEP(16, 4, 2) : SWEEP(16, 4, 1);
    if (ni <= 32) return two ? SWEEP(32, 4, 2) : SWEEP(32, 4, 1);
    return SWEEP(64, 4, 1);                                          // 128 VGPRs of running row: one row per wave
#undef SWEEP
}

constexpr int PERM_MAX = 4096;         // the longest permutation k_perm_check takes: one bit of LDS per column

// flag[0] = 0 when perm[0 .. K-1] is a permutation of 0 .. K-1 (every entry in range, none twice), else 1.  One workgroup.
__global__ __launch_bounds__(256) void k_perm_check(const int32_t* __restrict__ perm, int K, int* __restrict__ flag) {
    __shared__ unsigned seen[PERM_MAX / 32];
    for (int i = threadIdx.x; i < PERM_MAX / 32; i += blockDim.x) seen[i] = 0u;
    __syncthreads();
    int bad = 0;
    for (int j = threadIdx.x; j < K; j += blockDim.x) {
        const int p = perm[j];
        if (p < 0 || p >= K) bad = 1;
        else if (atomicOr(&seen[p >> 5], 1u << (p & 31)) & (1u << (p & 31))) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) flag[0] = bad;
}

// 0 when the device array perm is a permutation of 0 .. K-1 (1 <= K <= PERM_MAX); -1 with the message set when it is not, or the HIP
// error.  The flag is a device word of this file's own (one per device, allocated on first use), written by k_perm_check and read
// back ONCE: the call waits for the stream, so it cannot be part of a stream capture.
int check_perm(const char* who, const int32_t* perm, int64_t K, hipStream_t st) {
    constexpr int MAX_DEV = 16;
    static int* flags[MAX_DEV] = {};
    static std::mutex mu;
    char msg[160];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) { adalog_set_error(who, e); return (int)e; }
    if (dev < 0 || dev >= MAX_DEV) { adalog_set_error_msg("gptq: device ordinal beyond 15"); return -1; }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) {
        snprintf(msg, sizeof msg, "%s: the check of perm waits for the stream and cannot be captured into a graph", who);
        adalog_set_error_msg(msg);
        return -1;
    }
    std::lock_guard<std::mutex> lk(mu);                              // one check at a time reads the device's flag
    if (!flags[dev]) {
        int* p = nullptr;
        if ((e = hipMalloc(&p, sizeof(int))) != hipSuccess) { adalog_set_error(who, e); return (int)e; }
        flags[dev] = p;
    }
    adalog_launch<k_perm_check>("k_perm_check", 0, dim3(1), 256, 0, st, perm, (int)K, flags[dev]);
    int bad = 1;
    if ((e = hipGetLastError()) != hipSuccess || (e = hipMemcpyAsync(&bad, flags[dev], sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess
        || (e = hipStreamSynchronize(st)) != hipSuccess) {
        adalog_set_error(who, e);
        return (int)e;
    }
    if (bad) {
        snprintf(msg, sizeof msg, "%s: perm is not a permutation of 0 .. K-1 (an entry out of range, or one twice)", who);
        adalog_set_error_msg(msg);
        return -1;
    }
    return 0;
}

// out[i][j] = H[perm[i]][perm[j]]: a workgroup writes 256 consecutive elements of one row of out and gathers them from ONE row of H
__global__ __launch_bounds__(256) void k_permute_sym(const double* __restrict__ H, int K, int64_t ldh, const int32_t* __restrict__ perm,
                                                     double* __restrict__ out, int64_t ldo) {
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j < K) out[i * ldo + j] = H[perm[i] * ldh + perm[j]];
}

}  // namespace

extern "C" int adalog_gptq_sweep_ok(int64_t R, int64_t K) {
    return R >= 1 && R <= ((int64_t)1 << 31) && K >= 32 && K <= 4096 && K % 32 == 0;
}

extern "C" int adalog_gptq_sweep_f32(const float* w, int64_t R, int64_t K, int64_t ldw, const float* scale, const float* zero_point,
                                     int per_row, int n_bits, const double* U, int64_t ldu, float* what, uint8_t* codes,
                                     double* objective, void* stream) {
    ADALOG_ARG_CHECK(w && scale && zero_point && U && what, "gptq_sweep: null pointer");
    ADALOG_ARG_CHECK(n_bits >= 2 && n_bits <= 8, "gptq_sweep: n_bits must be in [2,8]");
    ADALOG_ARG_CHECK(adalog_gptq_sweep_ok(R, K), "gptq_sweep: unsupported sizes (R >= 1, K a multiple of 32 in [32, 4096])");
    ADALOG_ARG_CHECK(ldw >= K && ldu >= K, "gptq_sweep: bad sizes (ldw >= K, ldu >= K)");
    ADALOG_ARG_CHECK(per_row == 0 || per_row == 1, "gptq_sweep: per_row must be 0 or 1");
    const int rc = sweep(w, R, K, ldw, scale, zero_point, per_row, n_bits, U, ldu, nullptr, what, codes, objective, (hipStream_t)stream);
    if (rc) return rc;
    ADALOG_LAUNCH_CHECK("adalog_gptq_sweep_f32");
    return 0;
}

extern "C" int adalog_gptq_sweep_perm_f32(const float* w, int64_t R, int64_t K, int64_t ldw, const float* scale, const float* zero_point,
                                          int per_row, int n_bits, const double* U, int64_t ldu, const int32_t* perm, float* what,
                                          uint8_t* codes, double* objective, void* stream) {
    ADALOG_ARG_CHECK(w && scale && zero_point && U && what, "gptq_sweep_perm: null pointer");
    ADALOG_ARG_CHECK(perm, "gptq_sweep_perm: null perm");
    ADALOG_ARG_CHECK(n_bits >= 2 && n_bits <= 8, "gptq_sweep_perm: n_bits must be in [2,8]");
    ADALOG_ARG_CHECK(adalog_gptq_sweep_ok(R, K), "gptq_sweep_perm: unsupported sizes (R >= 1, K a multiple of 32 in [32, 4096])");
    ADALOG_ARG_CHECK(ldw >= K && ldu >= K, "gptq_sweep_perm: bad sizes (ldw >= K, ldu >= K)");
    ADALOG_ARG_CHECK(per_row == 0 || per_row == 1, "gptq_sweep_perm: per_row must be 0 or 1");
    static_assert(PERM_MAX >= 4096, "k_perm_check covers the sweep's K");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = check_perm("gptq_sweep_perm", perm, K, st)) return rc;      // an entry outside 0 .. K-1 would be a wild address
    if (const int rc = sweep(w, R, K, ldw, scale, zero_point, per_row, n_bits, U, ldu, perm, what, codes, objective, st)) return rc;
    ADALOG_LAUNCH_CHECK("adalog_gptq_sweep_perm_f32");
    return 0;
}

extern "C" int adalog_permute_sym_f64(const double* H, int64_t K, int64_t ldh, const int32_t* perm, double* out, int64_t ldo,
                                      void* stream) {
    ADALOG_ARG_CHECK(H && out, "permute_sym: null pointer");
    ADALOG_ARG_CHECK(perm, "permute_sym: null perm");
    ADALOG_ARG_CHECK(K >= 1 && K <= PERM_MAX, "permute_sym: unsupported size (1 <= K <= 4096)");
    ADALOG_ARG_CHECK(ldh >= K && ldo >= K, "permute_sym: bad sizes (ldh >= K, ldo >= K)");
    ADALOG_ARG_CHECK(H != out, "permute_sym: out must not be H");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = check_perm("permute_sym", perm, K, st)) return rc;
    if (const int rc = adalog_launch<k_permute_sym>("k_permute_sym", 0, dim3((unsigned)((K + 255) / 256), (unsigned)K), 256, 0, st, H, (int)K,
                                                    ldh, perm, out, ldo))
        return rc;
    ADALOG_LAUNCH_CHECK("adalog_permute_sym_f64");
    return 0;
}
