// Part of gemm_score.hip (one translation unit, included inside its anonymous namespace): shared operand / argument types and MFMA helpers of the scoring GEMM kernels.
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));

constexpr int BM = 128, BN = 128, BKB = 64;   // BKB: K-step in bytes

struct GemmArgs {
    const uint8_t* A; const uint8_t* B;
    int64_t sAc, sAg, sBc, sBg;      // byte strides between candidates / groups (0 = shared operand)
    int M, N; int64_t Kb;            // Kb = padded K in bytes: the row stride (multiple of 128; 64 for the streaming kernel)
    int64_t KbA;                     // mixed operands (bf16 rows x fp8 columns, k_gemm_grpk8): row stride of A in bytes; Kb is B's
    int64_t Kvb;                     // bytes of a row that can be non-zero (<= Kb)
    int C, G, gmod;
    const float* ref; int64_t ldr, sRg, ref_cs; int ref_div;
    const float* sa; int64_t sa_c, sa_g;
    const float* sb; int64_t sb_c, sb_g, sb_n;
    const float* bias; int64_t bi_c, bi_g, bi_n;
    const float* row_scale; const float* row_bias;   // optional per-ROW factor / offset (transposed activation searches)
    float* partial; int MT, NT, Npad;
    float* out; int64_t ldo, sOc, sOg;
    // quant_forward extras of the large-tile kernel's STORE epilogue (adalog_gemm_out_ex): out += addend (the residual stream, same
    // indexing as out), and two-level output groups -- group g at (g % out_gi) * sOg + (g / out_gi) * sOo (out_gi = 0: g * sOg):
    // softmax . v writes [B][N][H][D] storage directly, the transpose(1, 2) in front of the projection layer is a view
    const float* addend; int out_gi; int64_t sOo;
    float sa_mul;                    // constant folded into sa (e.g. 1/(4L-2) for AdaLog numerators)
    int reduce_cols;                 // 1: one partial per tile (sum over its columns) instead of one per column
    int order;                       // tile order (fastest index first): 0 = nt,mt,g,c  1 = nt,c,mt,g  2 = mt,nt,c,g
    double* wg_acc;                  // streaming kernel: per-workgroup fp64 column sums [workgroup][gmod][256] instead of
                                     // per-tile partials (searches that do not keep the column axis)
    int gm;                          // streaming kernel, order 2: m-tiles per L2 group (rows of A kept hot while n advances)
    int slab_U, slab_R;              // slab kernel: 32-row units per slab, units per workgroup (NT = slabs, MT = pieces);
                                     // group kernel: chunks per group, 32-column blocks per chunk
    // slab kernel, GEN form: the candidate operand is generated in the kernel from the fp32 activation
    const float* gen_x; int64_t gen_ldx; int gen_K;      // activation [tokens][gen_ldx], gen_K valid elements per row
    const float* gen_scale; const float* gen_zp;         // the candidates' (scale, zero point): element [cand * gen_sc + row * gen_sn]
    int64_t gen_sc, gen_sn;                              //   (1, 0): per-tensor activation candidates [ref_div]; (rows, 1): weight candidates [ref_div][rows]
    int64_t gen_sg;                                      // window / group kernels, GEN form: stride between the groups of gen_x (rows gen_ldx apart)
    const uint32_t* gen_lut; const float* gen_q; int gen_nb; // log-base kernel: value table [gen_nb + 1][ref_div] (bf16 bits; row gen_nb = masked = 0), the bases q [ref_div]
    const float* gen_sa;                                 // optional device scalar folded into the column factor (the fixed operand's scale)
    float gen_qmax, gen_tie;                             // 2^bits - 1; |frac| above which the IEEE quotient decides the bin
    long long* timeline;             // profiling only (tools/gemm_lab.hip): 8 cycle stamps per workgroup, else nullptr
    // ROWMAP form of the large-tile kernel (adalog_gemm_out_gen_rows): row r of the generated A operand is read from row
    // a_rows[r % row_period] + (r / row_period) * row_period of gen_x, and the STORE epilogue writes (and reads the addend of) row
    // o_rows[r % row_period] + (r / row_period) * row_period; a null map is the identity
    const int* a_rows; const int* o_rows; int row_period;
};
#if defined(GEMM_LAB_TIMELINE)   // tools/lab only: the stamp stores would otherwise cost waits in the production kernel
#define TL_STAMP(i) do { if (p.timeline && threadIdx.x == 0) p.timeline[(size_t)lid * 8 + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define TL_STAMP(i) do { } while (0)
#endif
static long long* g_timeline = nullptr;   // set only by the lab harness, which includes this file
static int g_slab_override = -1;          // lab harness: force the slab kernel off (0) / on (1) per call

__device__ __forceinline__ int swz(int row, int slot) { return row * BKB + ((slot ^ ((row >> 2) & 3)) << 4); }

template <int DT> struct Acc { typedef v16f type; };
template <> struct Acc<0> { typedef v16i type; };

template <int DT>
__device__ __forceinline__ void mma(const uint4& a, const uint4& b, typename Acc<DT>::type& c) {
    if constexpr (DT == 0) {
        c = __builtin_amdgcn_mfma_i32_32x32x32_i8(*reinterpret_cast<const v4i*>(&a), *reinterpret_cast<const v4i*>(&b), c, 0, 0, 0);
    } else if constexpr (DT == 1) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const v8bf*>(&a), *reinterpret_cast<const v8bf*>(&b), c, 0, 0, 0);
    } else {
        const float* af = reinterpret_cast<const float*>(&a);
        const float* bf = reinterpret_cast<const float*>(&b);
#pragma unroll
        for (int s = 0; s < 4; ++s) c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], bf[s], c, 0, 0, 0);
    }
}

// fp8 (e4m3) operands, 64 K-bytes per instruction: lane = (row, K half) holds 32 bytes.  Any fixed permutation of K is
// fine as long as A and B share it, so the two 16-byte fragments a lane reads for the int8 path are simply concatenated.
typedef int v8i __attribute__((ext_vector_type(8)));
__device__ __forceinline__ v16f mma_fp8x64(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1, v16f c) {
    const v8i a = {(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
    const v8i b = {(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);   // scales 2^0
}

// fp8 e4m3 -> bf16 in registers (exact; gfx950 v_cvt_scalef32_pk_bf16_fp8: two values per instruction, scale 1): the mixed-operand
// kernels keep their candidate columns as fp8 in HBM / LDS and feed the bf16 MFMA.
typedef __bf16 v2bf __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t fp8x2_bf16(uint32_t w, bool hi) {
    const v2bf r = hi ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w, 1.0f, false);
    return *reinterpret_cast<const uint32_t*>(&r);
}
__device__ __forceinline__ void fp8x16_bf16(const uint4& s, uint4& lo, uint4& hi) {
    lo.x = fp8x2_bf16(s.x, false); lo.y = fp8x2_bf16(s.x, true); lo.z = fp8x2_bf16(s.y, false); lo.w = fp8x2_bf16(s.y, true);
    hi.x = fp8x2_bf16(s.z, false); hi.y = fp8x2_bf16(s.z, true); hi.z = fp8x2_bf16(s.w, false); hi.w = fp8x2_bf16(s.w, true);
}

