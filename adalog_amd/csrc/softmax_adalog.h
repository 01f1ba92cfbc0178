// The row arithmetic of quant_forward's softmax + post-softmax AdaLog quantiser, shared by the kernels that restate it:
// k_softmax_adalog_pack_t (operand.hip: scores from HBM, packed operand to HBM) and k_attn_core / k_attn_core_long (attn_core.hip:
// both stay on the chip).
// One definition, so that the two routes quantise the same fp32 probabilities bit for bit.
#pragma once
#include "common.h"

// bf16 value table of the post-softmax AdaLog quantiser in LDS (levels2 + 2 entries, built by the whole workgroup; the caller
// synchronises): entry k = mant[(k q) % 37] * 2^-((k q) / 37), the masked levels (k >= levels2, or an exponent past 100) = 0.
__device__ __forceinline__ void adalog_value_lut_bf16(unsigned short* s_lut, int levels2, float qf, const float* mant) {
    const int lw = levels2 + 2;
    for (int k = threadIdx.x; k < lw; k += blockDim.x) {
        const int kqv = k * (int)qf;
        const int t = kqv / ADALOG_R, j = kqv - t * ADALOG_R;
        const float v = (k >= levels2 || t > 100) ? 0.0f : ldexpf(mant[j], -t);
        s_lut[k] = (unsigned short)(__float_as_uint(v) >> 16);
    }
}

// ATen's softmax_warp_forward over one row held by a wavefront, operation for operation: element k = lane + 64 it in el[it]
// (-inf where k is past the row); max over `it`, then the xor butterfly 32, 16, .., 1; el[it] = exp(el[it] - max) summed per lane in
// `it` order, then the same butterfly.  Returns the sum; the probabilities are el[it] / sum.
// NS slots per lane: 4 (rows of <= 256), 8 (<= 512) or 16 (<= 1024) -- ATen's WARP_ITERATIONS for the row's next power of two.  ATen keeps
// this per-warp form up to 1024 elements per row; past that it switches to a block-wide softmax with another summation order, so
// 1024 is where the restatement ends.  A row shorter than 64 (NS - 1) + 1 only adds exact zeros (exp(-inf)) to the ATen order.
template <int NS>
__device__ __forceinline__ float softmax_warp_row(float (&el)[NS]) {
    static_assert(NS == 4 || NS == 8 || NS == 16, "softmax_warp_row: 4, 8 or 16 slots per lane");
    float mx = el[0];
#pragma unroll
    for (int it = 1; it < NS; ++it) mx = mx < el[it] ? el[it] : mx;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float b = __shfl_xor(mx, o); mx = mx < b ? b : mx; }
    float sum = 0.0f;
#pragma unroll
    for (int it = 0; it < NS; ++it) { el[it] = expf(el[it] - mx); sum += el[it]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum = sum + __shfl_xor(sum, o);
    return sum;
}

// the probability e / sum through the quantiser (matmul.py:337-343: u clamped to [1e-15, 1], levels clamped to levels2 + 1 = masked)
// as bf16 bits out of the table above
__device__ __forceinline__ unsigned short adalog_prob_bf16(float e, float sum, float sc, float inv_s, float qf, float rq37, int levels2,
                                                           const unsigned short* s_lut) {
    const float pr = e / sum;
    float kk = adalog_k_fast(pr, sc, inv_s, qf, rq37, true);
    kk = (kk == kk) ? fminf(fmaxf(kk, 0.0f), (float)(levels2 + 1)) : (float)(levels2 + 1);
    return s_lut[(int)kk];
}
