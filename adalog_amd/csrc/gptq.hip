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
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PF = 4;     // steps a block's own U values are read ahead of their use

__device__ __forceinline__ double bcast(double v, int lane) {        // lane: wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

template <int NI_MAX, int G, int RPW>
__global__ __launch_bounds__(256) void k_gptq_sweep(const float* __restrict__ w, int64_t R, int K, int64_t ldw,
                                                    const float* __restrict__ scale, const float* __restrict__ zp, int per_row,
                                                    float qmax, const double* __restrict__ U, int64_t ldu,
                                                    float* __restrict__ what, uint8_t* __restrict__ codes,
                                                    double* __restrict__ objective) {
    static_assert(NI_MAX % G == 0, "slots come in whole groups");
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t row0 = wave * RPW;
    if (row0 >= R) return;                                           // (whole waves leave: nothing below synchronises)
    const int ni = (K + 63) >> 6;
    // a lane's element offset inside a slot's 64 columns of U; in the last slot, which may be half full (K is a multiple of 32), the
    // lanes beyond K read the row's last element: in bounds, never used
    const int last = K - 1 - (ni - 1) * 64;
    const unsigned vtail = (unsigned)(lane < last ? lane : last);

    double run[RPW][NI_MAX];
    float s[RPW], z[RPW];
    int64_t rows[RPW];
    double obj[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        rows[r] = row0 + r < R ? row0 + r : R - 1;                   // a wave's rows beyond R repeat the last row and store nothing
        const int64_t pi = per_row ? rows[r] : 0;
        s[r] = scale[pi];
        z[r] = rintf(zp[pi]);
        obj[r] = 0.0;
#pragma unroll
        for (int i = 0; i < NI_MAX; ++i) {
            const int col = i * 64 + lane;
            run[r][i] = col < K ? (double)w[rows[r] * ldw + col] : 0.0;
        }
    }

    for (int i = 0; i < ni; ++i) {
        const int j0 = i * 64;
        const int nl = K - j0 < 64 ? K - j0 : 64;                    // 32 or 64 (K is a multiple of 32)
        const int col = j0 + lane;
        const unsigned uoff = i == ni - 1 ? vtail : (unsigned)lane;
        double cur[RPW], ev[RPW];
        float qv[RPW], cv[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            cur[r] = 0.0; ev[r] = 0.0; qv[r] = 0.0f; cv[r] = 0.0f;
#pragma unroll
            for (int ii = 0; ii < NI_MAX; ++ii)
                if (ii == i) cur[r] = run[r][ii];
        }
        // ---- 1. the block's own steps
        double un[PF];
#pragma unroll
        for (int t = 0; t < PF; ++t) un[t] = (U + ((int64_t)(j0 + t) * ldu + j0))[uoff];   // (nl >= 32 > PF)
        for (int l0 = 0; l0 < nl; l0 += PF) {
#pragma unroll
            for (int t = 0; t < PF; ++t) {
                const int l = l0 + t;
                const double u = un[t];                                                // U[j0 + l][col]
                if (l + PF < nl) un[t] = (U + ((int64_t)(j0 + l + PF) * ldu + j0))[uoff];
                const double d = bcast(u, l);                                          // U[j][j]
#pragma unroll
                for (int r = 0; r < RPW; ++r) {
                    const double x = bcast(cur[r], l);
                    const float c = uni_bin((float)x, s[r], z[r], qmax);
                    const float q = (c - z[r]) * s[r];
                    const double e = (x - (double)q) / d;
                    obj[r] = obj[r] + e * e;
                    if (lane == l) { qv[r] = q; cv[r] = c; ev[r] = e; }
                    if (lane > l) cur[r] = cur[r] - e * u;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r)
            if (col < K && row0 + r < R) {
                what[rows[r] * (int64_t)K + col] = qv[r];
                if (codes) codes[rows[r] * (int64_t)K + col] = (uint8_t)(int)cv[r];
            }
        // ---- 2. the block's errors onto the later slots
#pragma unroll
        for (int g = 0; g < NI_MAX / G; ++g) {
            // a slot ii of the group with i < ii < ni exists; i + 1 < ni also says that block i is full: rows j0 .. j0 + 63 of U exist
            if (i + 1 < ni && g * G + G - 1 > i && g * G < ni) {
                // A wave-uniform base and a 32-bit lane offset per slot; a slot beyond K reads the last slot's values, which are never
                // used.  The empty asm keeps these few values from being hoisted out of the loop over blocks for every group at once
                // (one VGPR and two SGPRs per slot, live across the whole kernel: more registers than the running row itself).
                int last_slot = ni - 1;
                unsigned full = (unsigned)lane, tail = vtail;
                asm volatile("" : "+s"(last_slot), "+v"(full), "+v"(tail));
                int sl[G];
                unsigned off[G];
#pragma unroll
                for (int a = 0; a < G; ++a) {
                    sl[a] = g * G + a < last_slot ? g * G + a : last_slot;
                    off[a] = sl[a] == last_slot ? tail : full;
                }
                const double* urow = U + (int64_t)j0 * ldu;
#pragma unroll 4
                for (int l = 0; l < 64; ++l, urow += ldu) {
                    double e[RPW];
#pragma unroll
                    for (int r = 0; r < RPW; ++r) e[r] = bcast(ev[r], l);
#pragma unroll
                    for (int a = 0; a < G; ++a) {
                        const double u = (urow + sl[a] * 64)[off[a]];
#pragma unroll
                        for (int r = 0; r < RPW; ++r) run[r][g * G + a] = run[r][g * G + a] - e[r] * u;
                    }
                }
            }
        }
    }
    if (objective && lane == 0) {
#pragma unroll
        for (int r = 0; r < RPW; ++r)
            if (row0 + r < R) objective[rows[r]] = obj[r];
    }
}

template <int NI_MAX, int G, int RPW>
int launch_sweep(const float* w, int64_t R, int64_t K, int64_t ldw, const float* scale, const float* zp, int per_row, int n_bits,
                 const double* U, int64_t ldu, float* what, uint8_t* codes, double* objective, hipStream_t st) {
    const int64_t waves = (R + RPW - 1) / RPW;
    const int wpb = waves >= 1024 ? 4 : 1;                           // few rows: one wave per workgroup spreads them over the CUs
    const dim3 grid((unsigned)((waves + wpb - 1) / wpb));
    return adalog_launch<k_gptq_sweep<NI_MAX, G, RPW>>("k_gptq_sweep", 0, grid, 64 * wpb, 0, st, w, R, (int)K, ldw, scale, zp, per_row,
                                                       (float)((1 << n_bits) - 1), U, ldu, what, codes, objective);
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
    hipStream_t st = (hipStream_t)stream;
    const int ni = (int)((K + 63) >> 6);
    const bool two = R > 2048;                                       // two rows per wave halve the reads of U once the SIMDs are full
    int rc;
#define SWEEP(NI_MAX, G, RPW) launch_sweep<NI_MAX, G, RPW>(w, R, K, ldw, scale, zero_point, per_row, n_bits, U, ldu, what, codes, objective, st)
    if (ni <= 4) rc = two ? SWEEP(4, 1, 2) : SWEEP(4, 1, 1);
    else if (ni <= 8) rc = two ? SWEEP(8, 2, 2) : SWEEP(8, 2, 1);
    else if (ni <= 16) rc = two ? SWEEP(16, 4, 2) : SWEEP(16, 4, 1);
    else if (ni <= 32) rc = two ? SWEEP(32, 4, 2) : SWEEP(32, 4, 1);
    else rc = SWEEP(64, 4, 1);                                       // 128 VGPRs of running row: one row per wave
#undef SWEEP
    if (rc) return rc;
    ADALOG_LAUNCH_CHECK("adalog_gptq_sweep_f32");
    return 0;
}
