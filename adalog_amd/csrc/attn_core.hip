// quant_forward of the attention core in ONE launch (reference utils/wrap_net.py:23-30 / :41-51 with both products in quant_forward,
// quant_layers/matmul.py:43-45): q . k^T on the int8 MFMA, scale (or relative-position bias + shift mask), softmax, the post-softmax
// AdaLog quantiser and softmax . v on the bf16 MFMA, from the packed operands of adalog_attn_split_pack to the heads-last
// output [B][N][H][D].  The scores and the quantised probabilities live in LDS only: what gemm_out(I8) -> softmax_(bias_)adalog_pack
// -> gemm_out(BF16, heads_last) hand from launch to launch through HBM (deit_small, 32 images: 49 MB written and read per block).
//
// The result equals those three launches bit for bit, because every step is exact or restated in their order:
//   scores   int8 MFMA, int32 accumulators (exact in any order; only the ceil(D / 32) K-steps that hold codes are issued), then the
//            STORE epilogue of k_gemm_cand: s = (float)acc * (sq * 1 * sk); s += 0;
//   softmax  k_softmax_adalog_pack_t's restatement of ATen's softmax_warp_forward and the quantiser, through the SAME device functions
//            (softmax_adalog.h): a wavefront per row, element k on lane k % 64, slot k / 64;
//   . v      v_mfma_f32_32x32x16_bf16, one accumulator chain per output element over the 16-element K chunks 0 .. Kp / 16 - 1 in
//            ascending order with k_gemm_cand's fragment layout (lanes 0-31: elements 0-7 of the chunk, lanes 32-63: elements 8-15),
//            then o = (float)acc * (a_scale * sa_mul * sv); o += 0.  No split-K.
//
// A workgroup (4 wavefronts) owns one group g = image (or window) * H + head and a tile of TM * 32 query rows:
//   1. wavefront w forms the score columns [64 w, 64 w + 64) of the tile (operand fragments straight from global memory: a row of qp /
//      kp is read once per workgroup and wavefront) and writes them as fp32 into the LDS tile [TM * 32][Kp + 4];
//   2. the wavefronts take the tile's rows in turn: softmax + quantiser, the bf16 row written over the head of its own fp32 row (a
//      row is in registers before its first bf16 value is stored; rows are Kp + 4 floats apart, so the 16-byte fragment reads of step
//      3 fall on different banks);
//   3. wavefront (i, j) multiplies row block i of the probabilities by the 32 channels j of v (fragments of vp from global memory,
//      requested before step 2 so that they arrive under it) and stores its 32 x 32 piece of out.
// LDS: TM * 32 * (Kp + 4) * 4 bytes + the 258-entry value table: <= 65.5 KiB for 64 rows x 256 keys, 33 KiB for 32 rows -- two to four
// workgroups per CU next to <= 128 VGPRs.  The row tile is 32 rows unless 64-row tiles pad no more (N = 197: 7 x 32 = 224 against 256).
#include "common.h"
#include "softmax_adalog.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));

struct AttnCoreArgs {
    const int8_t* qp; const int8_t* kp;                  // int8 [G][N][128]: D codes, then zeros
    const unsigned short* vp;                            // bf16 bits [G][D][Kp]: v transposed, zero beyond N
    int64_t G; int N, D, H, gmod, MT;                    // MT: row tiles per group
    int Kp;                                              // keys padded to a multiple of 64 (rows of vp, rows of the probability operand)
    const float* sq; const float* sk; const float* sv; int pg;   // scales of the q / k / v quantisers: element (g % gmod) * pg
    float mul;                                           // plain form: scores * mul in front of the softmax
    const float* a_scale; const float* qv; const float* mant; int levels2;   // post-softmax AdaLog quantiser (device scalars, 37 numerators)
    float sa_mul;                                        // constant folded into a_scale in the second product's epilogue
    const float* table; const int64_t* index;            // BIAS: relative_position_bias_table [*][H], relative_position_index [N][N]
    const float* mask; int nW;                           // BIAS: shift mask [nW][N][N] or null
    float* out;                                          // fp32 [G / H][N][H][D]
    int64_t bid0;                                        // first (group, row tile) pair of this launch
};

// The steps the two kernels share.  Each is written once, so that the two kernels cannot drift apart in the orders that the header
// comment names (STORE epilogue, softmax + quantiser, softmax . v epilogue).

// the two 16-byte code fragments (K-steps 0 and 1) of this lane's row of a packed int8 operand; a K-step without codes, or a row
// that nobody multiplies (`live` false), is zero and is not read
__device__ __forceinline__ void load_codes(v4i (&f)[2], const int8_t* row, bool live, int nks) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) f[ks] = (live && ks < nks) ? *reinterpret_cast<const v4i*>(row + ks * 32) : v4i{0, 0, 0, 0};
}

// one 32 x 32 block of scores: the ceil(D / 32) K-steps that hold codes, then the STORE epilogue of k_gemm_cand into the LDS tile S
// (rows `ld` floats apart) at rows [row0, row0 + 32) x columns [col0, col0 + 32)
__device__ __forceinline__ void score_block(const v4i (&af)[2], const v4i (&bf)[2], int nks, float alpha, float* S, int ld, int row0,
                                            int col0, int frow, int fkg) {
    v16i acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[0], bf[0], acc, 0, 0, 0);
    if (nks > 1) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[1], bf[1], acc, 0, 0, 0);
    float* sp = S + (row0 + 4 * fkg) * ld + col0 + frow;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float s = (float)acc[r] * alpha;
        s += 0.0f;
        sp[((r & 3) + 8 * (r >> 2)) * ld] = s;
    }
}

// softmax + quantiser over the tile's `rows` rows (query rows m0 ..), a wavefront per row, the WAVES wavefronts of the workgroup in
// turn; NS slots per lane (softmax_adalog.h).  The bf16 row replaces the head of its own fp32 row, zero from N to Kp.
template <int NS, bool BIAS, int WAVES>
__device__ __forceinline__ void softmax_quant_rows(const AttnCoreArgs& a, float* S, int ld, const unsigned short* s_lut, int64_t g, int h,
                                                   int m0, int rows, int w, int lane, float qf, float sc) {
    const int N = a.N, Kp = a.Kp;
    const float inv_s = __builtin_amdgcn_rcpf(sc), rq37 = 37.0f / qf;
    const float* mk = nullptr;
    if constexpr (BIAS) { if (a.mask) mk = a.mask + ((g / a.H) % a.nW) * (int64_t)N * N; }
    for (int rl = w; rl < rows; rl += WAVES) {
        float* srow = S + rl * ld;
        float el[NS];
#pragma unroll
        for (int it = 0; it < NS; ++it) {
            const int k = lane + 64 * it;
            float e = -__builtin_inff();
            if (k < N) {
                const float s = srow[k];
                if constexpr (BIAS) {
                    const int64_t rc = (int64_t)(m0 + rl) * N + k;
                    e = s + a.table[a.index[rc] * a.H + h];
                    if (mk) e = e + mk[rc];
                } else {
                    e = s * a.mul;
                }
            }
            el[it] = e;
        }
        const float sum = softmax_warp_row(el);
        unsigned short* prow = reinterpret_cast<unsigned short*>(srow);
#pragma unroll
        for (int it = 0; it < NS; ++it) {
            const int k = lane + 64 * it;
            if (k >= Kp) break;
            prow[k] = k < N ? adalog_prob_bf16(el[it], sum, sc, inv_s, qf, rq37, a.levels2, s_lut) : (unsigned short)0;
        }
    }
}

// the epilogue of softmax . v: o = (float)acc * (a_scale * sa_mul * sv); o += 0, stored heads-last [B][N][H][D] -- this lane's 16
// values are rows row0 + 4 fkg + {0..3, 8..11, 16..19, 24..27} of channel `col`
__device__ __forceinline__ void pv_store(const AttnCoreArgs& a, const v16f& acc, int64_t g, int gh, int h, int row0, int col, int fkg) {
    const int N = a.N, D = a.D;
    const float alpha = a.a_scale[0] * a.sa_mul * a.sv[gh * a.pg];
    float* og = a.out + ((g / a.H) * (int64_t)N * a.H + h) * D + col;
    if (col < D) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row0 + 4 * fkg + (r & 3) + 8 * (r >> 2);
            if (row < N) {
                float o = acc[r] * alpha;
                o += 0.0f;
                og[(int64_t)row * a.H * D] = o;
            }
        }
    }
}

template <int TM, bool BIAS>
__global__ __launch_bounds__(256) void k_attn_core(AttnCoreArgs a) {
    constexpr int BMR = 32 * TM;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int ld = a.Kp + 4;                                           // floats between the rows of the score tile
    float* S = reinterpret_cast<float*>(smem);
    unsigned short* s_lut = reinterpret_cast<unsigned short*>(smem + (size_t)BMR * ld * 4);

    const int64_t bid = a.bid0 + blockIdx.x;
    const int64_t g = bid / a.MT;
    const int mt = (int)(bid - g * a.MT);
    const int m0 = mt * BMR;
    const int gh = (int)(g % a.gmod), h = (int)(g % a.H);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int frow = lane & 31, fkg = lane >> 5;
    const int N = a.N, D = a.D, Kp = a.Kp;

    const float qf = a.qv[0], sc = a.a_scale[0];
    adalog_value_lut_bf16(s_lut, a.levels2, qf, a.mant);

    // ---- 1. scores: wavefront w takes key columns [64 w, 64 w + 64)
    if (w * 64 < N) {
        const int nks = (D + 31) >> 5;                                 // 32-byte K-steps that hold codes
        const int8_t* qg = a.qp + g * (int64_t)N * 128 + fkg * 16;
        const int8_t* kg = a.kp + g * (int64_t)N * 128 + fkg * 16;
        v4i af[TM][2], bf[2][2];
#pragma unroll
        for (int i = 0; i < TM; ++i) load_codes(af[i], qg + (int64_t)min(m0 + i * 32 + frow, N - 1) * 128, true, nks);
#pragma unroll
        for (int j = 0; j < 2; ++j) load_codes(bf[j], kg + (int64_t)min(w * 64 + j * 32 + frow, N - 1) * 128, true, nks);
        const float alpha = a.sq[gh * a.pg] * 1.0f * a.sk[gh * a.pg];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) score_block(af[i], bf[j], nks, alpha, S, ld, i * 32, w * 64 + j * 32, frow, fkg);
    }

    // ---- 3 (requests): this wavefront's fragments of v, all K chunks
    constexpr int NJ = 4 / TM;                                         // 32-channel blocks the wavefronts of a row block are spread over
    const int pi = w / NJ, pj = w % NJ;
    const bool pv_live = pj * 32 < D;                                  // (TM = 1: wavefronts 2, 3 have no channels)
    const int nkv = Kp >> 4;
    uint4 vf[16];
    {
        const int d = min(pj * 32 + frow, D - 1);
        const unsigned short* vg = a.vp + (g * D + d) * (int64_t)Kp + fkg * 8;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks)
            vf[ks] = (pv_live && ks < nkv) ? *reinterpret_cast<const uint4*>(vg + ks * 16) : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();

    // ---- 2. softmax + quantiser, a wavefront per row; the bf16 row replaces the head of the fp32 row
    softmax_quant_rows<4, BIAS, 4>(a, S, ld, s_lut, g, h, m0, min(BMR, N - m0), w, lane, qf, sc);
    __syncthreads();

    // ---- 3. softmax . v: wavefront (pi, pj) -> rows [32 pi, 32 pi + 32) x channels [32 pj, 32 pj + 32)
    if (pv_live && m0 + pi * 32 < N) {
        v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const uint8_t* pa = smem + (size_t)(pi * 32 + frow) * ld * 4 + fkg * 16;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            if (ks < nkv) {
                const uint4 pf = *reinterpret_cast<const uint4*>(pa + ks * 32);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const v8bf*>(&pf), *reinterpret_cast<const v8bf*>(&vf[ks]),
                                                              acc, 0, 0, 0);
            }
        }
        pv_store(a, acc, g, gh, h, m0 + pi * 32, pj * 32 + frow, fkg);
    }
}

// The plain form for rows of up to 1024 keys (a ViT / DeiT at 384 px: 577 tokens).  k_attn_core gives every wavefront one 64-column key
// block and holds all of v's K chunks in registers, which ends at 256 keys; here a workgroup of LONG_WAVES wavefronts owns one group
// and 32 query rows, and
//   1. the wavefronts take the 64-column key blocks in turn (block kb goes to wavefront kb % LONG_WAVES; the next block's fragments of
//      kp are requested before the current block's MFMAs) and write the fp32 score tile [32][Kp + 4] into LDS: 32 * 1028 * 4 =
//      131 584 bytes at 1024 keys plus the value table, inside the 160 KiB of a CU;
//   2. softmax + quantiser, a wavefront per row, NS = 4 / 8 / 16 slots per lane for rows of <= 256 / 512 / 1024 (softmax_adalog.h: the
//      slot count ATen uses for the row's next power of two), the bf16 row over the head of its own fp32 row as above;
//   3. wavefront j < ceil(D / 32) multiplies the 32 rows by the 32 channels j of v.  v's fragments come from global memory eight K
//      chunks (128 keys) at a time, the next eight requested before the MFMAs of the current eight (the first eight before step 2).
//      The chunks go in ascending order into ONE accumulator chain per output element, as in k_gemm_cand: no split-K, same bits.
constexpr int LONG_WAVES = 8;
template <int NS>
__global__ __launch_bounds__(64 * LONG_WAVES) void k_attn_core_long(AttnCoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int ld = a.Kp + 4;                                           // floats between the rows of the score tile
    float* S = reinterpret_cast<float*>(smem);
    unsigned short* s_lut = reinterpret_cast<unsigned short*>(smem + (size_t)32 * ld * 4);

    const int64_t bid = a.bid0 + blockIdx.x;
    const int64_t g = bid / a.MT;
    const int m0 = (int)(bid - g * a.MT) * 32;
    const int gh = (int)(g % a.gmod), h = (int)(g % a.H);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int frow = lane & 31, fkg = lane >> 5;
    const int N = a.N, D = a.D, Kp = a.Kp;

    const float qf = a.qv[0], sc = a.a_scale[0];
    adalog_value_lut_bf16(s_lut, a.levels2, qf, a.mant);

    // ---- 1. scores: wavefront w takes the key blocks w, w + LONG_WAVES, ..
    {
        const int nks = (D + 31) >> 5;                                 // 32-byte K-steps that hold codes
        const int nkb = (N + 63) >> 6;                                 // key blocks that hold keys
        const int8_t* kg = a.kp + g * (int64_t)N * 128 + fkg * 16;
        v4i af[2], bf[2][2];
        load_codes(af, a.qp + (g * (int64_t)N + min(m0 + frow, N - 1)) * 128 + fkg * 16, true, nks);
#pragma unroll
        for (int j = 0; j < 2; ++j) load_codes(bf[j], kg + (int64_t)min(w * 64 + j * 32 + frow, N - 1) * 128, w < nkb, nks);
        const float alpha = a.sq[gh * a.pg] * 1.0f * a.sk[gh * a.pg];
        for (int kb = w; kb < nkb; kb += LONG_WAVES) {
            v4i bn[2][2];
            const bool more = kb + LONG_WAVES < nkb;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                load_codes(bn[j], kg + (int64_t)min((kb + LONG_WAVES) * 64 + j * 32 + frow, N - 1) * 128, more, nks);
#pragma unroll
            for (int j = 0; j < 2; ++j) score_block(af, bf[j], nks, alpha, S, ld, 0, kb * 64 + j * 32, frow, fkg);   // (columns < Kp = 64 nkb)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) bf[j][ks] = bn[j][ks];
        }
    }

    // ---- 3 (requests): the first eight K chunks of this wavefront's fragments of v
    const bool pv_live = w * 32 < D;
    const int nkv = Kp >> 4;
    const unsigned short* vg = a.vp + (g * D + min(w * 32 + frow, D - 1)) * (int64_t)Kp + fkg * 8;
    uint4 vf[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) vf[i] = (pv_live && i < nkv) ? *reinterpret_cast<const uint4*>(vg + i * 16) : make_uint4(0, 0, 0, 0);
    __syncthreads();

    // ---- 2. softmax + quantiser, a wavefront per row; the bf16 row replaces the head of the fp32 row
    softmax_quant_rows<NS, false, LONG_WAVES>(a, S, ld, s_lut, g, h, m0, min(32, N - m0), w, lane, qf, sc);
    __syncthreads();

    // ---- 3. softmax . v: wavefront w -> the tile's 32 rows x channels [32 w, 32 w + 32)
    if (pv_live) {
        v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const uint8_t* pa = smem + (size_t)frow * ld * 4 + fkg * 16;
        for (int k0 = 0; k0 < nkv; k0 += 8) {
            uint4 vn[8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
                vn[i] = k0 + 8 + i < nkv ? *reinterpret_cast<const uint4*>(vg + (k0 + 8 + i) * 16) : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (k0 + i < nkv) {
                    const uint4 pf = *reinterpret_cast<const uint4*>(pa + (k0 + i) * 32);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const v8bf*>(&pf), *reinterpret_cast<const v8bf*>(&vf[i]),
                                                                  acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) vf[i] = vn[i];
        }
        pv_store(a, acc, g, gh, h, m0, w * 32 + frow, fkg);
    }
}

// ---- host: one path for the two entry points

bool head_dim_ok(int D) { return D == 16 || D == 32 || D == 48 || D == 64; }

// the argument checks of adalog_attn_core (`name` "attn_core", n_max 256) and adalog_attn_core_long ("attn_core_long", 1024, no
// table / index / mask): 0, or -1 with "<name>: <what is wrong>" as the error
int attn_core_check(const char* name, int n_max, const void* qp, const void* kp, const void* vp, int64_t G, int N, int D, int H, int gmod,
                    int64_t Np, const float* q_scale, const float* k_scale, const float* v_scale, int pg, const float* a_scale,
                    const float* qv, int n_bits, const float* mant37, const float* table, const int64_t* index, const float* mask, int nW,
                    const float* out) {
    char n_range[48];
    snprintf(n_range, sizeof(n_range), "1 <= N <= %d tokens per group", n_max);
    const char* what =
        !(qp && kp && vp && q_scale && k_scale && v_scale && a_scale && qv && mant37 && out) ? "null pointer"
        : !head_dim_ok(D) ? "head dimension D must be 16, 32, 48 or 64"
        : !(N >= 1 && N <= n_max) ? n_range
        : Np != (int64_t)((N + 63) / 64) * 64 ? "Np (rows of vp) must be N rounded up to a multiple of 64"
        : !(n_bits >= 2 && n_bits <= 7) ? "n_bits must be in [2,7]"
        : !(G >= 1 && H >= 1 && gmod >= 1 && G % H == 0 && G % gmod == 0 && (pg == 0 || pg == 1))
            ? "G must be a multiple of H and of gmod, pg 0 or 1"
        : !((table != nullptr) == (index != nullptr) && (!mask || (table && nW >= 1)))
            ? "table and index go together; a mask needs them and nW >= 1"
        : !(((uintptr_t)qp & 15) == 0 && ((uintptr_t)kp & 15) == 0 && ((uintptr_t)vp & 15) == 0) ? "packed operands must be 16-byte aligned"
        : nullptr;
    if (!what) return 0;
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", name, what);
    adalog_set_error_msg(msg);
    return -1;
}

// the kernels' arguments from the (checked) arguments of an entry point; the grid's part (MT, bid0) is attn_core_launch's
AttnCoreArgs attn_core_args(const void* qp, const void* kp, const void* vp, int64_t G, int N, int D, int H, int gmod, int64_t Np,
                            const float* q_scale, const float* k_scale, const float* v_scale, int pg, float mul, const float* a_scale,
                            const float* qv, int n_bits, const float* mant37, float sa_mul, const float* table, const int64_t* index,
                            const float* mask, int nW, float* out) {
    AttnCoreArgs a{};
    a.qp = (const int8_t*)qp; a.kp = (const int8_t*)kp; a.vp = (const unsigned short*)vp;
    a.G = G; a.N = N; a.D = D; a.H = H; a.gmod = gmod; a.Kp = (int)Np;
    a.sq = q_scale; a.sk = k_scale; a.sv = v_scale; a.pg = pg; a.mul = mul;
    a.a_scale = a_scale; a.qv = qv; a.mant = mant37; a.levels2 = 1 << n_bits; a.sa_mul = sa_mul;
    a.table = table; a.index = index; a.mask = mask; a.nW = nW; a.out = out;
    return a;
}

// Launches KERNEL (`threads` per workgroup, tile_rows query rows per workgroup) over the flattened (group, row tile) grid, split far
// below the grid limit, after raising its dynamic-LDS limit to lds_max once per device.  0, or the HIP error (recorded under `entry`).
template <void (*KERNEL)(AttnCoreArgs)>
int attn_core_launch(const char* entry, AttnCoreArgs a, int tile_rows, int threads, int lds_max, hipStream_t st) {
    if (const int e = adalog_lds_limit<KERNEL>(lds_max)) return e;
    a.MT = cdiv(a.N, tile_rows);
    const size_t shm = (size_t)tile_rows * (a.Kp + 4) * 4 + 264 * sizeof(unsigned short);
    const int64_t total = a.G * a.MT, per_launch = (int64_t)1 << 30;
    for (int64_t b0 = 0; b0 < total; b0 += per_launch) {
        a.bid0 = b0;
        const int64_t nb = total - b0 < per_launch ? total - b0 : per_launch;
        hipLaunchKernelGGL(KERNEL, dim3((unsigned)nb), dim3(threads), shm, st, a);
    }
    ADALOG_LAUNCH_CHECK(entry);
    return 0;
}

}  // namespace

// the shapes adalog_attn_core takes: 1 <= N <= 256 keys (the bound of adalog_softmax_adalog_pack_bf16), head dimension 16, 32, 48 or 64
extern "C" int adalog_attn_core_supported(int N, int D) { return (N >= 1 && N <= 256 && head_dim_ok(D)) ? 1 : 0; }

extern "C" int adalog_attn_core(const void* qp, const void* kp, const void* vp, int64_t G, int N, int D, int H, int gmod, int64_t Np,
                                const float* q_scale, const float* k_scale, const float* v_scale, int pg, float mul,
                                const float* a_scale, const float* qv, int n_bits, const float* mant37, float sa_mul,
                                const float* table, const int64_t* index, const float* mask, int nW, float* out, void* stream) {
    if (attn_core_check("attn_core", 256, qp, kp, vp, G, N, D, H, gmod, Np, q_scale, k_scale, v_scale, pg, a_scale, qv, n_bits, mant37,
                        table, index, mask, nW, out))
        return -1;
    const int tm = ((N + 31) / 32) * 32 < ((N + 63) / 64) * 64 ? 1 : 2;     // 64-row tiles only when they pad no more than 32-row tiles
    const AttnCoreArgs a = attn_core_args(qp, kp, vp, G, N, D, H, gmod, Np, q_scale, k_scale, v_scale, pg, mul, a_scale, qv, n_bits,
                                          mant37, sa_mul, table, index, mask, nW, out);
    const char* entry = "adalog_attn_core";
    hipStream_t st = (hipStream_t)stream;
    adalog_note_kernel("k_attn_core");
    if (table) return tm == 2 ? attn_core_launch<k_attn_core<2, true>>(entry, a, 64, 256, 68 * 1024, st)
                              : attn_core_launch<k_attn_core<1, true>>(entry, a, 32, 256, 68 * 1024, st);
    return tm == 2 ? attn_core_launch<k_attn_core<2, false>>(entry, a, 64, 256, 68 * 1024, st)
                   : attn_core_launch<k_attn_core<1, false>>(entry, a, 32, 256, 68 * 1024, st);
}

// the shapes adalog_attn_core_long takes: 1 <= N <= 1024 keys (as far as ATen's per-warp softmax goes), head dimension 16, 32, 48 or 64
extern "C" int adalog_attn_core_long_supported(int N, int D) { return (N >= 1 && N <= 1024 && head_dim_ok(D)) ? 1 : 0; }

// The plain form (softmax(scores * mul): ViT / DeiT) of adalog_attn_core for up to 1024 tokens per group; same operands, same bits as
// gemm_out(I8) -> adalog_softmax_adalog_pack(_long)_bf16 -> gemm_out(BF16, heads_last).  LDS per workgroup: 32 (Np + 4) 4 + 528 bytes.
extern "C" int adalog_attn_core_long(const void* qp, const void* kp, const void* vp, int64_t G, int N, int D, int H, int gmod, int64_t Np,
                                     const float* q_scale, const float* k_scale, const float* v_scale, int pg, float mul,
                                     const float* a_scale, const float* qv, int n_bits, const float* mant37, float sa_mul, float* out,
                                     void* stream) {
    if (attn_core_check("attn_core_long", 1024, qp, kp, vp, G, N, D, H, gmod, Np, q_scale, k_scale, v_scale, pg, a_scale, qv, n_bits,
                        mant37, nullptr, nullptr, nullptr, 0, out))
        return -1;
    const AttnCoreArgs a = attn_core_args(qp, kp, vp, G, N, D, H, gmod, Np, q_scale, k_scale, v_scale, pg, mul, a_scale, qv, n_bits,
                                          mant37, sa_mul, nullptr, nullptr, nullptr, 0, out);
    const char* entry = "adalog_attn_core_long";
    const int threads = 64 * LONG_WAVES;
    hipStream_t st = (hipStream_t)stream;
    adalog_note_kernel("k_attn_core_long");
    if (N <= 256) return attn_core_launch<k_attn_core_long<4>>(entry, a, 32, threads, 136 * 1024, st);
    if (N <= 512) return attn_core_launch<k_attn_core_long<8>>(entry, a, 32, threads, 136 * 1024, st);
    return attn_core_launch<k_attn_core_long<16>>(entry, a, 32, threads, 136 * 1024, st);
}
