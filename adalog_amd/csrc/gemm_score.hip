// K7/K8/K11-K15 -- candidate-scoring GEMM with a fused squared-error epilogue, on the CDNA4 matrix cores.
//
// Replaces, for every scoring call of the reference's searches
//   quant_layers/linear.py:355-384 (_search_best_w_scale), :394-423 (_search_best_a_scale),
//   :816-848/:856-890/:898-931 (post-GELU AdaLog searches), matmul.py:135-163/:173-201/:321-351, conv.py:226-255,
// the sequence  F.linear / @ / F.conv2d  ->  out_sim[.., P, ..] in HBM  ->  (raw_out - out_sim)**2  ->  mean/sum,
// by ONE kernel per call: D = A.B^T on MFMA from packed operands (operand.hip), then in registers
//   out = D * (sa * sb[col]) + bias[col];   e = ref - out;   column sums of e*e over the tile's rows,
// so only per-tile score partials ever reach HBM (the reference materialises out_sim: 3.7 GB for deit_small qkv).
// A second tiny kernel adds the partials in fp64 in a fixed order (deterministic, SURVEY "hard parts").
//
// Data types:  0 = int8  (v_mfma_i32_32x32x32_i8,  exact integer dot products)
//              3 = fp8   (v_mfma_scale_f32_32x32x64_f8f6f4, e4m3: operands q - z in [-15, 15] of <= 4-bit layers are exact,
//                         sums < 2^24 exact in the fp32 accumulator; same rate as int8, no cvt in the epilogue)
//              1 = bf16  (v_mfma_f32_32x32x16_bf16, AdaLog operand m*2^-t and integer operand exact in bf16)
//              2 = fp32  (v_mfma_f32_32x32x2_f32,   conv patch-embed with unquantised 8-bit input)
// Five kernels live here (DESIGN.md section 4 has the measurements that led from one to the next):
//   k_gemm_slab    -- int8 searches with K <= 384 bytes: 256 candidate columns resident in LDS, the fixed operand
//                     streamed wave-privately past them, column sums in registers, no barrier in the main loop;
//   k_gemm_grp     -- attention q.k^T searches (one K-step, many small groups): 7 consumer waves with register-resident
//                     row fragments + 1 LDS-DMA loader wave;
//   k_gemm_stream  -- every other search (candidates in the GEMM columns, reference rows contiguous): persistent
//                     workgroups, LDS-DMA ring streaming across tiles, packed-fp32 epilogue, per-workgroup fp64 sums;
//   k_gemm_cand    -- quant_forward (stores the product) and the launches k_gemm_stream does not take
//                     (k_gemm_cand_glds is its LDS-DMA variant): (64..256) x 256 tile, 128-byte K-steps;
//   k_gemm_score   -- candidates in a grid dimension (C > 1): 128 x 128 tile, 64-byte K-steps.
// All stage operands through LDS with a 16-byte-slot XOR swizzle (0 bank conflicts measured) and order workgroups so that
// tiles sharing an operand run on one XCD (its L2).
#include "common.h"
#include "fpcs_tail.h"
#include <stdlib.h>

// The quantisation kernels are compiled without FMA contraction (bin indices must round like the reference); this file
// holds no bin-defining arithmetic, so the epilogues may fuse multiply-adds.
#pragma clang fp contract(fast)

namespace {

#include "gemm_types.inc"
#include "gemm_k_basic.inc"
#include "gemm_k_stream.inc"
#include "gemm_k_slab.inc"
#include "gemm_k_grp.inc"
#include "gemm_k_avw.inc"
#include "gemm_finish.inc"

}  // namespace

static int device_cus() {
    static int n_cu = 0;
    if (!n_cu) {
        int dev = 0; hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
        if (n_cu <= 0) n_cu = 256;
    }
    return n_cu;
}

// ---- tile selection shared by launch, layout query and finish
// quant_forward (store form): the products of a forward pass are small -- fc2 of deit_small is 25 x 2 tiles of 256 x 256 on 256 CUs.
// Largest row tile that still gives every CU its two workgroups; 64-row tiles otherwise.  Measured per product of a deit_small
// forward (32 images, us per launch at 256- / 128- / 64-row tiles): fc2 66 / 39 / 26, softmax.v 29 / 28 / 16, proj - / 22 / 13,
// fc1 - / 31 / 21, qkv - / 20 / 17, q.k^T 13 / 15 / 12 (profiles/r06_notes.md).
static int pick_tm_out(int M, int64_t col_tiles_x_groups) {
    if (const char* e = getenv("ADALOG_GEMM_TM")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) return v; }
    const int64_t want = 2 * (int64_t)device_cus();
    const int tms[3] = {4, 2, 1};
    for (int i = 0; i < 3; ++i)
        if ((int64_t)cdiv(M, 64 * tms[i]) * col_tiles_x_groups >= want) return tms[i];
    return 1;
}

static int pick_tm(int M, bool scoring) {
    // largest row tile whose padding waste stays within 10 % of the best achievable.  The scoring epilogue keeps more
    // state than the store epilogue: with TM = 4 (128 accumulator VGPRs) it spills, so scoring launches use TM <= 2.
    if (const char* e = getenv("ADALOG_GEMM_TM")) {             // tuning knob for experiments (1, 2 or 4)
        const int v = atoi(e);
        if (v == 1 || v == 2 || (v == 4 && !scoring)) return v;
    }
    double best = 0.0;
    int tms[3] = {scoring ? 2 : 4, 2, 1};
    double util[3];
    for (int i = 0; i < 3; ++i) {
        const int bm = 64 * tms[i];
        util[i] = (double)M / ((double)cdiv(M, bm) * bm);
        if (util[i] > best) best = util[i];
    }
    for (int i = 0; i < 3; ++i)
        if (util[i] >= 0.9 * best) return tms[i];
    return 1;
}

struct Layout { int big, tm, wide, MT, NT, Npad, c_eff, n_eff, stream, acc, wgs, slab, slab_U, slab_R, slab_nb; int64_t elems; };

// Wide (one workgroup per CU, 192/256-row tile) form of the streaming kernel: from 8 K-steps on, where the L2 -> LDS path
// bounds the main loop (measured: K = 768 int8 -- vit_base / deit_base -- 0.39 -> 0.44 of peak, a calibration 4.5 % shorter;
// K = 512 -- swin stage 2 -- +4 %; below that the un-overlapped epilogue of the larger tile costs more than it saves).
static int pick_wide(int M, int64_t kvalid_bytes) {
    static const int use_wide = getenv("ADALOG_GEMM_WIDE") ? atoi(getenv("ADALOG_GEMM_WIDE")) : 1;
    static const int min_k = getenv("ADALOG_GEMM_WIDE_MINK") ? atoi(getenv("ADALOG_GEMM_WIDE_MINK")) : 512;
    if (!use_wide || kvalid_bytes < min_k || M < 192) return 0;
    const int64_t pad4 = (int64_t)cdiv(M, 256) * 256, pad3 = (int64_t)cdiv(M, 192) * 192, pad2 = (int64_t)cdiv(M, 128) * 128;
    const int ri = pad4 <= pad3 + pad3 / 32 ? 4 : 3;                      // 256 rows unless 192 pads > 3 % less
    const int64_t padw = ri == 4 ? pad4 : pad3;
    return padw <= pad2 + pad2 / 8 ? ri : 0;                              // not if it pads > 12 % more than 128-row tiles
}

// reduce_cols with ref_div > 1 asks for per-workgroup accumulation, which only the streaming kernel provides: when that
// kernel is not eligible the launch falls back to per-tile partials (candidate innermost), and the layout says so.
static Layout layout_of(int M, int N, int C, int G, int gmod, int ref_div, int reduce_cols, bool scoring = true,
                        int64_t kvalid_bytes = 0, int64_t kb = 0, bool ref_transposed = false, int dtype = -1, bool gen = false) {
    static const int use_stream = getenv("ADALOG_GEMM_STREAM") ? atoi(getenv("ADALOG_GEMM_STREAM")) : 1;
    static const int use_wgacc = getenv("ADALOG_GEMM_WGACC") ? atoi(getenv("ADALOG_GEMM_WGACC")) : 1;
    Layout L{};
    L.big = (C == 1);
    L.tm = L.big ? (scoring ? pick_tm(M, scoring) : pick_tm_out(M, (int64_t)cdiv(N, 256) * G)) : 2;
    const bool cand_cols = L.big && scoring && ref_transposed && (ref_div == 64 || ref_div == 128 || ref_div == 256);
    if (cand_cols && use_stream) {
        L.wide = pick_wide(M, kvalid_bytes);
        if (L.wide) L.tm = L.wide;
    }
    L.stream = cand_cols && use_stream && (L.tm <= 2 || L.wide) && (int64_t)(64 * L.tm + BN2) * kb < ((int64_t)1 << 31);
    if (!L.stream && L.wide) { L.wide = 0; L.tm = pick_tm(M, scoring); }
    // Slab kernel: int8 or fp8 storage, one group, 2..6 K-steps (the 256-column slab is <= 96 KiB), whole 32-row units, at least three
    // units per wave and slab, and a streamed operand small enough for the caches.
    static const int use_slab = getenv("ADALOG_GEMM_SLAB") ? atoi(getenv("ADALOG_GEMM_SLAB")) : 1;
    // (the GEN form -- no packed operand, no packer launch -- pays from one unit per wave and slab on: attn.proj's 384 rows)
    static const int slab_min_m_env = getenv("ADALOG_GEMM_SLAB_MINM") ? atoi(getenv("ADALOG_GEMM_SLAB_MINM")) : 768;
    const int slab_min_m = gen ? 256 : slab_min_m_env;
    // streamed (fixed) operand: every workgroup walks all of it past its resident slab, from L2 or the Infinity Cache (16 MiB:
    // swin stage 0's 100 352 tokens x 128 B -- those launches ran on the streaming kernel at 0.26 of peak, 0.43 here)
    static const int64_t slab_max_bytes = getenv("ADALOG_GEMM_SLAB_MAXB") ? atoll(getenv("ADALOG_GEMM_SLAB_MAXB")) : ((int64_t)16 << 20);
    // 256-column slabs up to 6 K-steps; 128-column slabs up to 12 (K = 512 / 768: swin stage 2, vit_base) when a slab still holds
    // whole reference columns (64 or 128 candidates)
    static const int use_slab128 = getenv("ADALOG_GEMM_SLAB128") ? atoi(getenv("ADALOG_GEMM_SLAB128")) : 1;
    const bool ok128 = use_slab128 && kb <= 12 * BK3 && (ref_div == 64 || ref_div == 128);
    const int slab_nb = kb <= 6 * BK3 ? 8 : (ok128 ? 4 : 0);       // (128-column slabs at K = 384 were measured: +57 ms per calibration)
    if (L.stream && (g_slab_override >= 0 ? g_slab_override : use_slab) && (dtype == 0 || dtype == 3) && G == 1 && slab_nb != 0 && kvalid_bytes > BK3 && M % 32 == 0 && M >= slab_min_m &&
        (int64_t)M * kb <= slab_max_bytes && (int64_t)cdiv(N, 32 * slab_nb) * (M / 32) < ((int64_t)1 << 30)) {
        const int SBN = 32 * slab_nb;
        L.slab_nb = slab_nb;
        L.slab = 1;
        L.slab_U = M / 32;
        L.NT = cdiv(N, SBN);
        const int64_t units = (int64_t)L.NT * L.slab_U;
        L.slab_R = (int)(cdiv(cdiv(units, (int64_t)device_cus()), (int64_t)8) * 8);
        L.wgs = (int)cdiv(units, (int64_t)L.slab_R);
        L.MT = cdiv(L.slab_U, L.slab_R) + 1;                 // pieces a slab can be cut into by the range boundaries
        L.n_eff = N / ref_div;
        L.c_eff = ref_div;
        L.acc = reduce_cols && use_wgacc;
        L.Npad = cdiv(L.n_eff, 64) * 64;
        L.elems = L.acc ? (int64_t)2 * L.wgs * gmod * BN2 : (int64_t)L.c_eff * G * L.MT * L.Npad;
        L.wide = 0; L.tm = 2;
        return L;
    }
    const int bm = L.big ? 64 * L.tm : BM, bn = L.big ? BN2 : BN;
    L.MT = cdiv(M, bm);
    L.NT = cdiv(N, bn);
    L.n_eff = ref_div > 1 ? N / ref_div : N;
    L.c_eff = ref_div > 1 ? ref_div : C;
    const int64_t tiles = (int64_t)L.MT * L.NT * G * C;
    const int64_t want = (int64_t)(L.wide ? 1 : 2) * device_cus();
    L.wgs = (int)(tiles < want ? tiles : want);
    L.acc = L.stream && reduce_cols && ref_div > 1 && use_wgacc;
    const int red = reduce_cols && ref_div == 1;
    L.Npad = red ? L.NT : (ref_div > 1 ? cdiv(L.n_eff, 64) * 64 : L.NT * bn);
    L.elems = L.acc ? (int64_t)2 * L.wgs * gmod * BN2 : (int64_t)L.c_eff * G * L.MT * L.Npad;
    return L;
}

// The reference comes in columns of 64, 128 or 256 candidates
static bool ref_div_ok(int N, int ref_div) { return (ref_div == 64 || ref_div == 128 || ref_div == 256) && N % ref_div == 0; }

// GEN form of the attention searches (adalog_gemm_score_gen): the candidate operand B is not read but generated in the kernel
// from the fp32 tensor x [G][N / ref_div][K] with the candidates' (sb, zp) pairs
struct MmGen { const float* x; int64_t ldx, sg; const float* zp; int n_bits; };
// extras of the STORE epilogue (GemmArgs: addend, out_gi, sOo)
struct MmOutEx { const float* addend; int out_gi; int64_t sOo; };

// One launch as its entry point describes it (strides in elements, 0 = shared; the argument lists of adalog_gemm_score and its
// relatives say what each field means).  Entry points fill it field by field: what they leave out is zero / null.
struct MmCall {
    int dtype; const void *A, *B; int64_t sAc, sAg, sBc, sBg;                 // operands
    int M, N; int64_t Kp, k_valid; int C, G, gmod;                            // sizes
    const float* ref; int64_t ldr, sRg, ref_cs; int ref_div;                  // reference
    const float* sa; int64_t sa_c, sa_g; float sa_mul;                        // epilogue: out = D * (sa * sa_mul * sb) + bias
    const float* sb; int64_t sb_c, sb_g, sb_n;
    const float* bias; int64_t bi_c, bi_g, bi_n;
    const float *row_scale, *row_bias;
    float* partial; int64_t partial_elems;                                    // outputs: score partials, or the stored product
    float* out; int64_t ldo, sOc, sOg;
    int order, reduce_cols; void* stream;                                     // options
    const MmGen* gen; const MmOutEx* ox;
};

// the launch the adalog_gemm_*_ok queries ask about: C = 1, transposed reference [G][N / ref_div][M], plain column factors, no bias
static MmCall shape_call(int dtype, int M, int N, int G, int gmod, int ref_div, int64_t k_valid, int64_t Kp, int reduce_cols) {
    MmCall c{};
    c.dtype = dtype; c.M = M; c.N = N; c.Kp = Kp; c.k_valid = k_valid; c.C = 1; c.G = G; c.gmod = gmod;
    c.ldr = 1; c.ref_cs = M; c.ref_div = ref_div; c.reduce_cols = reduce_cols;
    return c;
}

// bytes per element of A / of B (dtype 4: bf16 rows x fp8 columns, laid out like the bf16 launch)
static int esz_a(int dtype) { return (dtype == 0 || dtype == 3) ? 1 : (dtype == 1 || dtype == 4) ? 2 : 4; }
static int esz_b(int dtype) { return dtype == 4 ? 1 : esz_a(dtype); }

static Layout call_layout(const MmCall& c, bool ref_transposed) {
    const int es = esz_a(c.dtype);
    return layout_of(c.M, c.N, c.C, c.G, c.gmod, c.ref_div, c.reduce_cols, c.out == nullptr, (c.k_valid > 0 ? c.k_valid : c.Kp) * es, c.Kp * es,
                     ref_transposed, c.dtype == 4 ? 1 : c.dtype);
}

// ---- what each kernel family asks of a launch: the single place where a kernel's limits are written (kvb: valid K in bytes)
// the loader-wave group kernels, whatever their operands: 5..7 row blocks, many groups, per-head sums that fit LDS, plain column
// factors, a reference group within 32-bit addressing
static bool grp_shape_ok(const MmCall& c) {
    static const int use_grp = getenv("ADALOG_GEMM_GRP") ? atoi(getenv("ADALOG_GEMM_GRP")) : 1;
    return use_grp && c.M > 128 && c.M <= 224 && c.G >= 8 && c.gmod <= 16 && !c.bias && !c.row_scale && c.sb_n == 0 && ref_div_ok(c.N, c.ref_div) &&
           (int64_t)(c.N / c.ref_div) * c.ref_cs * 4 < ((int64_t)1 << 31);
}
// ... and the window kernels: at most 64 rows, hundreds of groups or more, at least as many waves as heads per image (every
// participating wave owns one head), a reference slice that fits a wave's LDS
static bool win_shape_ok(const MmCall& c, int wgs) {
    static const int use_win = getenv("ADALOG_GEMM_WIN") ? atoi(getenv("ADALOG_GEMM_WIN")) : 1;
    return use_win && c.M >= 4 && c.M <= 64 && c.G >= 256 && c.gmod <= 32 && !c.bias && !c.row_scale && c.sb_n == 0 && ref_div_ok(c.N, c.ref_div) &&
           c.N / c.ref_div <= 64 && wgs * 4 >= c.gmod && c.ref_cs >= c.M;
}
static bool byte_operands(const MmCall& c) { return c.dtype == 0 || c.dtype == 3; }
// the group kernel (it shares the streaming kernel's accumulator layout, so the layout query does not need to know): int8 or fp8,
// one K-step
static bool grp_ok(const MmCall& c, int64_t kvb) { return byte_operands(c) && kvb <= BK3 && grp_shape_ok(c); }
// ... its wave-private form: a switch, and every participating wave owns one head
static bool grpw_ok(const MmCall& c, int wgs) {
    static const int use_grpw = getenv("ADALOG_GEMM_GRPW") ? atoi(getenv("ADALOG_GEMM_GRPW")) : 1;
    return use_grpw != 0 && wgs * 4 >= c.gmod && c.ref_cs >= c.M;
}
// ... its several-K-steps form: bf16, exactly 7 K-steps (K = 193..224 elements: the 197 tokens of a 224 x 224 ViT)
static bool grpk_ok(const MmCall& c, int64_t kvb) { return c.dtype == 1 && kvb > 6 * BK3 && kvb <= 7 * BK3 && grp_shape_ok(c); }
// ... its mixed form (dtype 4: bf16 rows x fp8 columns): exactly 4 K-steps of 64 elements (K = 193..256)
static bool grpk8_ok(const MmCall& c) { return c.k_valid > 192 && c.k_valid <= 256 && grp_shape_ok(c); }
// ... the trimmed-K form of the mixed kernel (k_gemm_grpk8t): rows of 208 elements, K = 193..208
static bool grpk8t_ok(const MmCall& c) { return c.k_valid <= 208 && grpk8_ok(c); }
// the window kernel: int8 or fp8, one K-step
static bool win_ok(const MmCall& c, int64_t kvb, int wgs) { return byte_operands(c) && kvb <= BK3 && win_shape_ok(c, wgs); }
// ... mixed operands: K <= 64 elements (one 64-byte fp8 K-step against 128-byte bf16 rows)
static bool winb_ok(const MmCall& c, int wgs) { return c.k_valid >= 1 && c.k_valid <= 64 && win_shape_ok(c, wgs); }

// The kernel family a launch runs on.  R_NONE: mixed operands (dtype 4) of a shape none of their three families takes.
enum Route { R_NONE, R_SLAB, R_WIN, R_GRPW, R_GRP, R_GRPK, R_STREAM, R_GLDS, R_CAND, R_SCORE, R_MX_STREAM, R_MX_WIN, R_MX_GRPK8, R_MX_GRPK8T };

// THE route decision: the launch code, its argument checks and the adalog_gemm_*_ok queries (on which ops.py routes) all ask this
// function.  From the call (shape, operand type, epilogue options) and its Layout; first match wins:
//   slab -> window -> wave-private group -> barrier group -> 7-step group -> stream -> LDS-DMA cand -> cand -> C > 1 fallback,
// mixed operands: wide stream (K > 256) | window (K <= 64) | 4-step group, trimmed where the rows are 208 elements.
static Route route_of(const MmCall& c, const Layout& L) {
    const bool acc_search = L.stream && !c.out && L.acc;
    if (c.dtype == 4) {
        static const int use_mx = getenv("ADALOG_GEMM_STREAM_MX") ? atoi(getenv("ADALOG_GEMM_STREAM_MX")) : 1;
        if (c.k_valid > 256) return (use_mx && L.stream && L.wide && !L.slab) ? R_MX_STREAM : R_NONE;
        if (!acc_search) return R_NONE;
        if (c.k_valid <= 64) return winb_ok(c, L.wgs) ? R_MX_WIN : R_NONE;
        if (!grpk8_ok(c)) return R_NONE;
        return (c.Kp == 208 && grpk8t_ok(c)) ? R_MX_GRPK8T : R_MX_GRPK8;
    }
    const int64_t kvb = (c.k_valid > 0 ? c.k_valid : c.Kp) * esz_a(c.dtype);
    if (L.slab && !c.out) return R_SLAB;
    if (acc_search && win_ok(c, kvb, L.wgs)) return R_WIN;
    if (acc_search && grp_ok(c, kvb)) return grpw_ok(c, L.wgs) ? R_GRPW : R_GRP;
    if (acc_search && grpk_ok(c, kvb)) return R_GRPK;
    if (L.stream && !c.out) return R_STREAM;
    static const int use_glds = getenv("ADALOG_GEMM_GLDS") ? atoi(getenv("ADALOG_GEMM_GLDS")) : 1;   // LDS-DMA pipeline (default on)
    if (L.big && use_glds && !c.out && L.tm <= 2) return R_GLDS;
    return L.big ? R_CAND : R_SCORE;
}

// candidates per reference column -> 32-column blocks per reference column, as a compile-time constant: f(integral_constant<int, NJ>)
template <class F>
static int with_nj(int ref_div, F&& f) {
    return adalog_dispatch<64, 128, 256>(ref_div, [&](auto rd) { return f(std::integral_constant<int, decltype(rd)::value / 32>{}); });
}
// the slab kernels' instantiations: f(NREF, DT, NB) for fp8 / int8 storage, 256- / 128-column slabs of 1, 2, 4 / 1, 2 reference columns
template <class F>
static int with_slab(int dtype, int slab_nb, int ref_div, F&& f) {
    const int nref = 32 * slab_nb / ref_div;
    return adalog_dispatch<3, 0>(dtype, [&](auto dt) {
        return adalog_dispatch<8, 4>(slab_nb, [&](auto nb) {
            auto go = [&](auto nr) { return f(nr, dt, nb); };
            if constexpr (decltype(nb)::value == 8) return adalog_dispatch<1, 2, 4>(nref, go);
            else return adalog_dispatch<1, 2>(nref, go);
        });
    });
}
// their labels: form 0 = packed candidates, 1 = generated activation candidates, 2 = generated weight candidates
static const char* slab_label(int form, int dt, int nb) {
    static const char* const names[3][2][2] = {
        {{"k_gemm_slab<i8>", "k_gemm_slab128<i8>"}, {"k_gemm_slab<fp8>", "k_gemm_slab128<fp8>"}},
        {{"k_gemm_slab_gen<i8>", "k_gemm_slab128_gen<i8>"}, {"k_gemm_slab_gen<fp8>", "k_gemm_slab128_gen<fp8>"}},
        {{"k_gemm_slab_wgen<i8>", "k_gemm_slab128_wgen<i8>"}, {"k_gemm_slab_wgen<fp8>", "k_gemm_slab128_wgen<fp8>"}}};
    return names[form][dt == 3][nb != 8];
}
// dynamic LDS of a slab launch: the resident slab, the streamed operand's ring, reference and sums
static size_t slab_lds(int64_t kvb, int slab_nb) {
    const int nk = (int)((kvb + BK3 - 1) / BK3), SBN = 32 * slab_nb;
    return (size_t)nk * SBN * BK3 + 8 * 3 * 32 * BK3 + 8 * 192 * 4 + 8 * SBN * 4;
}
// items of the loader-wave group kernels: a group's NB 32-column blocks in chunks of CB (a multiple of 8: chunks start on a reference
// column), about three items per workgroup
static void grp_chunks(GemmArgs& p, int N, int wgs, int G) {
    const int NB = N / 32;
    const int nch0 = cdiv((int64_t)3 * wgs, G);
    const int CB = cdiv(cdiv(NB, nch0 < 1 ? 1 : nch0), 8) * 8;
    p.slab_R = CB; p.slab_U = cdiv(NB, CB);
}
// items of the wave-private kernels (a wave per item): a group's n reference columns in chunks, about three items per wave, at least
// min_chunks of them
static void wave_chunks(GemmArgs& p, int n, int wgs, int G, int min_chunks = 1) {
    int nch = (int)cdiv(3 * ((int64_t)wgs * 4), G);
    if (nch < min_chunks) nch = min_chunks;
    nch = nch < 1 ? 1 : nch > n ? n : nch;
    const int cbc = cdiv(n, nch);
    p.slab_R = cbc; p.slab_U = cdiv(n, cbc);
}
// m-tiles per group of the streaming kernel: the group's A rows are re-read once per n-tile (from L2 / the 256 MiB Infinity Cache), the
// B tiles stream from HBM once per GROUP -- with the candidate operand at 150..600 MB per launch that stream is what must not repeat:
// groups of <= 8 MiB of A rows (2 MiB, half of an XCD's L2, re-read vit_base's fc2 candidates 25 times: 4.16 -> 4.05 s per
// calibration, 3.99 at 64 MiB; deit_small -- its operand fits the Infinity Cache -- is indifferent up to 16 MiB and 2 % slower at 64)
static int stream_gm(const Layout& L, int64_t a_row_bytes) {
    static const int64_t grp_bytes = getenv("ADALOG_GEMM_GM_BYTES") ? atoll(getenv("ADALOG_GEMM_GM_BYTES")) : ((int64_t)8 << 20);
    int64_t gm = grp_bytes / ((int64_t)64 * L.tm * a_row_bytes);
    if (const char* e = getenv("ADALOG_GEMM_GM")) gm = atoi(e);
    return (int)(gm < 1 ? 1 : gm > L.MT ? L.MT : gm);
}

// The kernels' arguments from a call and its Layout, operands and strides in bytes.  Every route starts from this one fill and states
// its deviations after it.
static GemmArgs gemm_args(const MmCall& c, const Layout& L) {
    const int ea = esz_a(c.dtype), eb = esz_b(c.dtype);
    GemmArgs p{};
    p.A = (const uint8_t*)c.A; p.B = (const uint8_t*)c.B;
    p.sAc = c.sAc * ea; p.sAg = c.sAg * ea; p.sBc = c.sBc * eb; p.sBg = c.sBg * eb;
    p.M = c.M; p.N = c.N; p.Kb = c.Kp * eb; p.Kvb = (c.k_valid > 0 ? c.k_valid : c.Kp) * eb; p.C = c.C; p.G = c.G; p.gmod = c.gmod;
    p.ref = c.ref; p.ldr = c.ldr; p.sRg = c.sRg; p.ref_cs = c.ref_cs; p.ref_div = c.ref_div;
    p.sa = c.sa; p.sa_c = c.sa_c; p.sa_g = c.sa_g; p.sa_mul = c.sa_mul;
    p.sb = c.sb; p.sb_c = c.sb_c; p.sb_g = c.sb_g; p.sb_n = c.sb_n;
    p.bias = c.bias; p.bi_c = c.bi_c; p.bi_g = c.bi_g; p.bi_n = c.bi_n;
    p.row_scale = c.row_scale; p.row_bias = c.row_bias;
    p.MT = L.MT; p.NT = L.NT; p.Npad = L.Npad;
    p.order = c.order; p.reduce_cols = c.reduce_cols && c.ref_div == 1; p.timeline = g_timeline;
    p.partial = c.partial; p.out = c.out; p.ldo = c.ldo; p.sOc = c.sOc; p.sOg = c.sOg;
    if (c.ox) { p.addend = c.ox->addend; p.out_gi = c.ox->out_gi; p.sOo = c.ox->sOo; }
    if (L.acc) p.wg_acc = (double*)c.partial;
    return p;
}
// ... of the mixed families (dtype 4): the bf16 rows have their own length in bytes; scoring only, never timed in the lab
static GemmArgs gemm_args_mixed(const MmCall& c, const Layout& L) {
    GemmArgs p = gemm_args(c, L);
    p.KbA = c.Kp * 2; p.reduce_cols = 0; p.timeline = nullptr;
    p.row_scale = nullptr; p.ldo = 0; p.sOc = 0; p.sOg = 0;
    return p;
}

// M, N: GEMM rows / columns (N includes the candidate factor when ref_div > 1).  Outputs the partial-buffer layout
// [c_eff][G][MT][Npad] the kernel will write, for allocation and for adalog_finish_scores.
extern "C" int64_t adalog_gemm_score_layout(int M, int N, int C, int G, int gmod, int ref_div, int reduce_cols, int dtype,
                                            int64_t Kp, int64_t k_valid, int ref_transposed, int* MT, int* Npad, int* mode) {
    MmCall c = shape_call(dtype, M, N, G, gmod, ref_div, k_valid, Kp, reduce_cols);
    c.C = C;
    const Layout L = call_layout(c, ref_transposed != 0);
    if (MT) *MT = L.acc ? L.wgs : L.MT;
    if (Npad) *Npad = L.acc ? BN2 : L.Npad;
    if (mode) *mode = L.acc ? 2 : (ref_div > 1 ? 1 : 0);
    return L.elems;
}

// 1 when a scoring launch of this shape runs on the window kernel, i.e. when int8 / fp8 operands of K <= 32 may be packed
// with 32-byte rows (half the operand bytes of the 64-byte K-step padding).  C = 1, reduce_cols = 1, transposed reference.
extern "C" int adalog_gemm_win_ok(int dtype, int M, int N, int G, int gmod, int ref_div, int64_t k_valid) {
    if (!(dtype == 0 || dtype == 3) || k_valid > 32 || ref_div < 1 || N % ref_div != 0) return 0;
    const MmCall c = shape_call(dtype, M, N, G, gmod, ref_div, k_valid, 32, 1);
    return route_of(c, call_layout(c, true)) == R_WIN ? 1 : 0;
}

// the mixed launch of a shape with rows of Kp elements, and its route (R_NONE: not taken)
static Route mixed_route(int M, int N, int G, int gmod, int ref_div, int64_t k_valid, int64_t Kp) {
    if (ref_div < 1 || N % ref_div != 0 || k_valid < 1) return R_NONE;
    const MmCall c = shape_call(4, M, N, G, gmod, ref_div, k_valid, Kp, k_valid > 256 ? 0 : 1);
    return route_of(c, call_layout(c, true));
}

// 1 when adalog_gemm_score takes dtype 4 (A: bf16 rows, B: fp8 e4m3 candidate columns, both [..][Kp] with Kp = 256 elements) for
// this shape: the softmax.v weight search of a 197-token ViT (M = 197 attention rows, K = 197 keys) with <= 4-bit candidates; the
// windows of a Swin (K <= 64, Kp = 64); and a third family, the wide streaming kernel (one group or many), rows of any multiple of
// 64 elements: taken when the all-bf16 launch of this shape would run on the wide form (K >= 256 elements, M >= 192).
// C = 1, reduce_cols = 1, transposed reference.
extern "C" int adalog_gemm_mixed_ok(int M, int N, int G, int gmod, int ref_div, int64_t k_valid) {
    const int64_t Kp = k_valid > 256 ? (k_valid + 63) / 64 * 64 : k_valid <= 64 ? 64 : 256;
    return mixed_route(M, N, G, gmod, ref_div, k_valid, Kp) != R_NONE ? 1 : 0;
}

// Row length (elements) of the trimmed-K form of the mixed 197-token family, or 0 when the shape is not taken by it (then Kp = 256 as
// adalog_gemm_mixed_ok describes): both operands may be packed with rows of 208 elements (13 sixteen-element slots) for K = 193..208.
extern "C" int adalog_gemm_mixed_ktrim(int M, int N, int G, int gmod, int ref_div, int64_t k_valid) {
    return mixed_route(M, N, G, gmod, ref_div, k_valid, 208) == R_MX_GRPK8T ? 208 : 0;
}

static int gemm_score_impl(const MmCall& c) {
    const int dtype = c.dtype, M = c.M, N = c.N, C = c.C, G = c.G, gmod = c.gmod, ref_div = c.ref_div;
    const int64_t Kp = c.Kp, k_valid = c.k_valid;
    const MmGen* gen = c.gen;
    hipStream_t st = (hipStream_t)c.stream;
    ADALOG_ARG_CHECK(c.A && (c.B || gen) && c.sa && c.sb, "gemm_score: null operand/scale pointer");
    ADALOG_ARG_CHECK(!c.ox || (c.out && C == 1 && !c.row_scale && (c.ox->out_gi == 0 || (c.ox->out_gi > 0 && G % c.ox->out_gi == 0))),
                     "gemm_out_ex: the epilogue extras need out, C == 1 and an inner group count that divides G");
    ADALOG_ARG_CHECK(!gen || ((dtype == 0 || dtype == 3) && gen->x && gen->zp && k_valid > 0 && k_valid % 16 == 0 && k_valid <= 64 &&
                              gen->ldx % 4 == 0 && gen->sg % 4 == 0 && (((uintptr_t)gen->x) & 15) == 0),
                     "gemm_score_gen: int8 / fp8 candidates of K = 16, 32, 48 or 64 from a 16-byte aligned fp32 tensor");
    ADALOG_ARG_CHECK(dtype >= 0 && dtype <= 4, "gemm_score: dtype must be 0 (i8), 1 (bf16), 2 (f32), 3 (fp8 e4m3) or 4 (bf16 rows x fp8 columns)");
    ADALOG_ARG_CHECK(M >= 1 && N >= 1 && C >= 1 && G >= 1 && gmod >= 1 && G % gmod == 0 && ref_div >= 1, "gemm_score: bad sizes");
    if (dtype == 4 && k_valid > 256) {
        // mixed operands, streaming family: the wide persistent kernel with two 64-byte planes of bf16 rows per fp8 K-step
        ADALOG_ARG_CHECK(Kp % 64 == 0 && k_valid <= Kp && C == 1 && c.partial && c.ref && !c.out && c.ldr == 1 && !c.row_scale &&
                         adalog_gemm_mixed_ok(M, N, G, gmod, ref_div, k_valid),
                         "gemm_score: bf16 x fp8 operands, streaming family: Kp a multiple of 64, C = 1, transposed reference, a shape adalog_gemm_mixed_ok accepts");
        ADALOG_ARG_CHECK(c.order >= 0 && c.order <= 2, "gemm_score: order must be 0, 1 or 2");
        const Layout L = call_layout(c, true);
        ADALOG_ARG_CHECK(route_of(c, L) == R_MX_STREAM, "gemm_score: bf16 x fp8 operands: not a wide streaming shape");
        ADALOG_ARG_CHECK(((int64_t)(M - 1) * c.ldr + (int64_t)(L.n_eff - 1) * (c.ref_cs > 0 ? c.ref_cs : 1) < ((int64_t)1 << 31)),
                         "gemm_score: reference group exceeds 32-bit addressing");
        ADALOG_ARG_CHECK(c.partial_elems >= L.elems, "gemm_score: partial buffer too small");
        if (L.acc) ADALOG_ARG_CHECK(((uintptr_t)c.partial & 7) == 0, "gemm_score: accumulator buffer must be 8-byte aligned");
        GemmArgs p = gemm_args_mixed(c, L);
        p.gm = stream_gm(L, p.KbA);
        const size_t shm = (size_t)3 * (2 * 64 * L.tm + BN2) * BK3;
        if (const int e = adalog_dispatch<4, 3>(L.wide, [&](auto ri) {
                return adalog_launch<k_gemm_stream<1, decltype(ri)::value, 8, 3, true>>("k_gemm_stream<bf16xfp8>", 150 * 1024, (unsigned)L.wgs, 512,
                                                                                        shm, st, p);
            })) return e;
        ADALOG_LAUNCH_CHECK("adalog_gemm_score (bf16 x fp8, streaming)");
        return 0;
    }
    if (dtype == 4) {
        // mixed operands: one kernel, one shape family (adalog_gemm_mixed_ok)
        const bool window = k_valid > 0 && k_valid <= 64;
        const bool ktrim = !window && Kp == 208 && grpk8t_ok(c);
        ADALOG_ARG_CHECK((Kp == (window ? 64 : 256) || ktrim) && k_valid > 0 && C == 1 && c.partial && c.ref && !c.out && c.ldr == 1 && c.reduce_cols == 1 &&
                         adalog_gemm_mixed_ok(M, N, G, gmod, ref_div, k_valid),
                         "gemm_score: bf16 x fp8 operands are taken for the shapes adalog_gemm_mixed_ok accepts only (Kp = 64 or 256, or 208 where adalog_gemm_mixed_ktrim says so; C = 1, transposed reference)");
        const Layout L = call_layout(c, true);
        ADALOG_ARG_CHECK(route_of(c, L) == (window ? R_MX_WIN : ktrim ? R_MX_GRPK8T : R_MX_GRPK8),
                         "gemm_score: bf16 x fp8 operands: epilogue options not supported for this shape");
        ADALOG_ARG_CHECK(c.partial_elems >= L.elems && ((uintptr_t)c.partial & 7) == 0, "gemm_score: accumulator buffer too small or misaligned");
        GemmArgs p = gemm_args_mixed(c, L);
        p.bias = nullptr; p.bi_c = 0; p.bi_g = 0; p.bi_n = 0; p.row_bias = nullptr;     // the group / window kernels take no bias, no row vectors
        if (window) {
            const int n_eff = N / ref_div;
            const size_t ref_lds = (size_t)4 * n_eff * 64 * 4, acc_lds = (size_t)gmod * 256 * 8;
            const size_t shm_w = ref_lds > acc_lds ? ref_lds : acc_lds;
            if (const int e = with_nj(ref_div, [&](auto nj) {
                    return adalog_launch<k_gemm_winb<decltype(nj)::value>>("k_gemm_winb<bf16xfp8>", 80 * 1024, (unsigned)L.wgs, 256, shm_w, st, p);
                })) return e;
            ADALOG_LAUNCH_CHECK("adalog_gemm_score (bf16 x fp8, windows)");
            return 0;
        }
        grp_chunks(p, N, L.wgs, G);
        if (ktrim) {
            // rows of 13 sixteen-element slots: 13 MFMAs per block hold every non-zero product of K <= 200, 14 of K <= 208
            const size_t shm_t = (size_t)3 * 4 * 32 * 208 + (size_t)7 * ref_div * 4 + (size_t)gmod * 256 * 8;   // 3 stages of 4 blocks x 208 bytes
            if (const int e = with_nj(ref_div, [&](auto nj) {
                    constexpr int NJ = decltype(nj)::value;
                    return k_valid <= 200 ? adalog_launch<k_gemm_grpk8t<NJ, 13>>("k_gemm_grpk8t<13,bf16xfp8>", 160 * 1024, (unsigned)L.wgs, 512, shm_t, st, p)
                                          : adalog_launch<k_gemm_grpk8t<NJ, 14>>("k_gemm_grpk8t<14,bf16xfp8>", 160 * 1024, (unsigned)L.wgs, 512, shm_t, st, p);
                })) return e;
            ADALOG_LAUNCH_CHECK("adalog_gemm_score (bf16 x fp8, trimmed K)");
            return 0;
        }
        const size_t shm = (size_t)3 * 4 * 4 * 32 * BK3 + (size_t)7 * ref_div * 4 + (size_t)gmod * 256 * 8;   // 3 stages of 4 K-steps x 4 blocks
        if (const int e = with_nj(ref_div, [&](auto nj) {
                return adalog_launch<k_gemm_grpk8<decltype(nj)::value, 4>>("k_gemm_grpk8<bf16xfp8>", 160 * 1024, (unsigned)L.wgs, 512, shm, st, p);
            })) return e;
        ADALOG_LAUNCH_CHECK("adalog_gemm_score (bf16 x fp8)");
        return 0;
    }
    const int esz = esz_a(dtype);
    ADALOG_ARG_CHECK(Kp > 0 && ((Kp * esz) % BK3 == 0 || (Kp * esz == 32 && (dtype == 0 || dtype == 3))),
                     "gemm_score: padded K must be a multiple of 64 bytes (32-byte rows: int8 / fp8, window kernel only)");
    ADALOG_ARG_CHECK((c.partial != nullptr) == (c.ref != nullptr), "gemm_score: partial and ref go together");
    ADALOG_ARG_CHECK(c.partial || c.out, "gemm_score: nothing to produce");
    ADALOG_ARG_CHECK(c.order >= 0 && c.order <= 2, "gemm_score: order must be 0, 1 or 2");
    ADALOG_ARG_CHECK(ref_div == 1 || (C == 1 && N % ref_div == 0 && !c.out), "gemm_score: ref_div > 1 needs C == 1, N % ref_div == 0, no out");
    ADALOG_ARG_CHECK(!c.row_scale || (C == 1 && c.row_bias), "gemm_score: per-row scale needs C == 1 and a row_bias vector");
    ADALOG_ARG_CHECK(!(c.partial && c.out), "gemm_score: either score against ref or store out, not both");
    const Layout L = call_layout(c, c.ldr == 1 && c.ref != nullptr);
    ADALOG_ARG_CHECK(k_valid >= 0 && k_valid <= Kp, "gemm_score: k_valid must be in [0, Kp]");
    ADALOG_ARG_CHECK(!c.ref || ((int64_t)(M - 1) * c.ldr + (int64_t)(L.n_eff - 1) * (c.ref_cs > 0 ? c.ref_cs : 1) < ((int64_t)1 << 31)),
                     "gemm_score: reference group exceeds 32-bit addressing");
    if (c.partial) ADALOG_ARG_CHECK(c.partial_elems >= L.elems, "gemm_score: partial buffer too small");
    if (L.acc) ADALOG_ARG_CHECK(((uintptr_t)c.partial & 7) == 0, "gemm_score: accumulator buffer must be 8-byte aligned");
    GemmArgs p = gemm_args(c, L);
    const Route route = route_of(c, L);
    if (gen) {
        ADALOG_ARG_CHECK(route == R_WIN || route == R_GRPW, "gemm_score_gen: not a shape of the window / wave-private group kernels (adalog_gemm_score_gen_ok)");
        p.gen_x = gen->x; p.gen_ldx = gen->ldx; p.gen_sg = gen->sg; p.gen_K = (int)k_valid; p.gen_zp = gen->zp;
        p.gen_qmax = (float)((1 << gen->n_bits) - 1);
        const float tie = 6e-7f * (float)(1 << gen->n_bits);
        p.gen_tie = 0.5f - (tie > 1e-5f ? tie : 1e-5f);
    }
    const int64_t nwg = (int64_t)L.MT * L.NT * G * C;
    ADALOG_ARG_CHECK(nwg < (int64_t)1 << 31, "gemm_score: grid too large");
    const unsigned grid = (unsigned)nwg, wgs = (unsigned)L.wgs;
    ADALOG_ARG_CHECK((Kp * esz) % BK2 == 0 || (L.stream && !c.out),
                     "gemm_score: rows padded to 64 (not 128) bytes are taken by the streaming search kernel only");
    ADALOG_ARG_CHECK((Kp * esz) % BK3 == 0 || route == R_WIN, "gemm_score: 32-byte rows are taken by the window kernel only (adalog_gemm_win_ok)");
    ADALOG_ARG_CHECK(dtype != 3 || (L.stream && !c.out), "gemm_score: fp8 operands are taken by the streaming search kernel only (ref_div 64/128/256, transposed reference)");
    const int n_eff = N / ref_div;
    const size_t acc_lds = (size_t)gmod * 256 * 8;                    // per-head fp64 sums of the group / window kernels
    int e = 0;
    switch (route) {
    case R_SLAB: {
        // slab kernel: one workgroup per CU, each takes a contiguous range of (slab, unit) pairs
        p.slab_U = L.slab_U; p.slab_R = L.slab_R;
        const size_t shm = slab_lds(p.Kvb, L.slab_nb);
        // a slab that is not cut has unused pieces: they must read as zero
        if (!L.acc) {
            const hipError_t me = hipMemsetAsync(c.partial, 0, (size_t)L.elems * sizeof(float), st);
            if (me != hipSuccess) { adalog_set_error("adalog_gemm_score (clear partials)", me); return (int)me; }
        }
        e = with_slab(dtype, L.slab_nb, ref_div, [&](auto nr, auto dt, auto nb) {
            constexpr int NREF = decltype(nr)::value, DT = decltype(dt)::value, NB = decltype(nb)::value;
            return adalog_dispatch<true, false>(c.row_scale != nullptr, [&](auto rows) {
                return adalog_launch<k_gemm_slab<NREF, decltype(rows)::value, DT, NB>>(slab_label(0, DT, NB), 160 * 1024, wgs, 512, shm, st, p);
            });
        });
    } break;
    case R_WIN: {
        // window kernel (swin attention searches): a wave per group, same accumulator layout and workgroup count
        const size_t ref_lds = (size_t)4 * n_eff * 64 * 4, shm = ref_lds > acc_lds ? ref_lds : acc_lds;
        e = with_nj(ref_div, [&](auto nj) {
            constexpr int NJ = decltype(nj)::value;
            if (dtype == 3)
                return gen ? adalog_launch<k_gemm_win<NJ, 3, true>>("k_gemm_win_gen<fp8>", 80 * 1024, wgs, 256, shm, st, p)
                           : adalog_launch<k_gemm_win<NJ, 3>>("k_gemm_win<fp8>", 80 * 1024, wgs, 256, shm, st, p);
            return gen ? adalog_launch<k_gemm_win<NJ, 0, true>>("k_gemm_win_gen<i8>", 80 * 1024, wgs, 256, shm, st, p)
                       : adalog_launch<k_gemm_win<NJ, 0>>("k_gemm_win<i8>", 80 * 1024, wgs, 256, shm, st, p);
        });
    } break;
    case R_GRPW: {
        // wave-private group kernel (q.k^T searches): a wave per (group, chunk of reference columns), no barrier in the loop
        wave_chunks(p, n_eff, L.wgs, G);
        const size_t ref_lds = (size_t)4 * 2 * 224 * 4, shm = ref_lds > acc_lds ? ref_lds : acc_lds;
        e = with_nj(ref_div, [&](auto nj) {                           // (no LDS-limit call: 3.5 KiB, or gmod x 2 KiB <= 32 KiB)
            constexpr int NJ = decltype(nj)::value;
            if (dtype == 3)
                return gen ? adalog_launch<k_gemm_grpw<NJ, 3, true>>("k_gemm_grpw_gen<fp8>", 0, wgs, 256, shm, st, p)
                           : adalog_launch<k_gemm_grpw<NJ, 3>>("k_gemm_grpw<fp8>", 0, wgs, 256, shm, st, p);
            return gen ? adalog_launch<k_gemm_grpw<NJ, 0, true>>("k_gemm_grpw_gen<i8>", 0, wgs, 256, shm, st, p)
                       : adalog_launch<k_gemm_grpw<NJ, 0>>("k_gemm_grpw<i8>", 0, wgs, 256, shm, st, p);
        });
    } break;
    case R_GRP: {
        // group kernel (q.k^T searches): same accumulator layout and workgroup count as the streaming kernel
        grp_chunks(p, N, L.wgs, G);
        const size_t shm = (size_t)3 * 8 * 32 * BK3 + 7 * 256 * 4 + acc_lds;
        e = with_nj(ref_div, [&](auto nj) {
            constexpr int NJ = decltype(nj)::value;
            return dtype == 3 ? adalog_launch<k_gemm_grp<NJ, 3>>("k_gemm_grp<fp8>", 96 * 1024, wgs, 512, shm, st, p)
                              : adalog_launch<k_gemm_grp<NJ, 0>>("k_gemm_grp<i8>", 96 * 1024, wgs, 512, shm, st, p);
        });
    } break;
    case R_GRPK: {
        // group kernel, 7 K-steps (softmax.v weight search)
        grp_chunks(p, N, L.wgs, G);
        const size_t shm = (size_t)3 * 7 * 2 * 32 * BK3 + (size_t)7 * ref_div * 4 + acc_lds;
        e = with_nj(ref_div, [&](auto nj) {
            return adalog_launch<k_gemm_grpk<decltype(nj)::value, 7>>("k_gemm_grpk<bf16>", 160 * 1024, wgs, 512, shm, st, p);
        });
    } break;
    case R_STREAM: {
        // persistent streaming kernel: two (wide form: one) workgroups per CU walk the tile list
        p.gm = stream_gm(L, p.Kb);
        const size_t shm = (size_t)(L.wide ? 4 : 3) * (64 * L.tm + BN2) * BK3;
        // row tiles of 256 / 192 rows (wide form: 8 waves, 4 stages) or 128 / 64 rows (4 waves, 3 stages)
        e = adalog_dispatch<0, 1, 2, 3>(dtype, [&](auto dt) {
            return adalog_dispatch<4, 3, 2, 1>(L.wide ? L.wide : L.tm, [&](auto ri) {
                constexpr int DT = decltype(dt)::value, RI = decltype(ri)::value, NW = RI >= 3 ? 8 : 4, NS = RI >= 3 ? 4 : 3;
                return adalog_launch<k_gemm_stream<DT, RI, NW, NS>>(
                    DT == 0 ? "k_gemm_stream<i8>" : DT == 1 ? "k_gemm_stream<bf16>" : DT == 2 ? "k_gemm_stream<f32>" : "k_gemm_stream<fp8>",
                    (NS == 4 ? 128 : 80) * 1024, wgs, 64 * NW, shm, st, p);
            });
        });
    } break;
    case R_GLDS: {
        const size_t shm = (size_t)3 * (64 * L.tm + BN2) * BK2 + (512 + 256) * sizeof(float);
        e = adalog_dispatch<0, 1, 2>(dtype, [&](auto dt) {
            return adalog_dispatch<2, 1>(L.tm, [&](auto tm) {
                return adalog_launch<k_gemm_cand_glds<decltype(dt)::value, decltype(tm)::value>>("k_gemm_cand_glds", 160 * 1024, grid, 512, shm, st, p);
            });
        });
    } break;
    case R_CAND: {
        const size_t shm = (size_t)(64 * L.tm + BN2) * BK2 + (512 + 256) * sizeof(float);
        if (c.out && c.ox) ADALOG_ARG_CHECK(dtype == 0 || dtype == 1, "gemm_out_ex: int8 or bf16 operands");
        e = adalog_dispatch<4, 2, 1>(L.tm, [&](auto tm) {
            constexpr int TM = decltype(tm)::value;
            if (c.out && c.ox)        // the STORE form with the epilogue extras (int8 / bf16 operands)
                return adalog_dispatch<0, 1>(dtype, [&](auto dt) {
                    return adalog_launch<k_gemm_cand<decltype(dt)::value, TM, true, false, true>>("k_gemm_cand_ex", 72 * 1024, grid, 512, shm, st, p);
                });
            return adalog_dispatch<0, 1, 2>(dtype, [&](auto dt) {
                return adalog_dispatch<true, false>(c.out != nullptr, [&](auto store) {
                    return adalog_launch<k_gemm_cand<decltype(dt)::value, TM, decltype(store)::value>>("k_gemm_cand", 72 * 1024, grid, 512, shm, st, p);
                });
            });
        });
    } break;
    default: {
        ADALOG_ARG_CHECK(!c.row_scale, "gemm_score: per-row scale is only available with C == 1");
        e = adalog_dispatch<0, 1, 2>(dtype, [&](auto dt) {
            return adalog_dispatch<true, false>(c.out != nullptr, [&](auto store) {
                return adalog_launch<k_gemm_score<decltype(dt)::value, decltype(store)::value>>("k_gemm_score", 0, grid, 256, 0, st, p);
            });
        });
    } break;
    }
    if (e) return e;
    ADALOG_LAUNCH_CHECK("adalog_gemm_score");
    return 0;
}

extern "C" int adalog_gemm_score(int dtype, const void* A, const void* B, int64_t sAc, int64_t sAg, int64_t sBc,
                                 int64_t sBg, int M, int N, int64_t Kp, int64_t k_valid, int C, int G, int gmod, const float* ref,
                                 int64_t ldr, int64_t sRg, int64_t ref_cs, int ref_div, const float* sa, int64_t sa_c,
                                 int64_t sa_g, float sa_mul, const float* sb, int64_t sb_c, int64_t sb_g, int64_t sb_n,
                                 const float* bias, int64_t bi_c, int64_t bi_g, int64_t bi_n, const float* row_scale,
                                 const float* row_bias, float* partial, int64_t partial_elems, float* out, int64_t ldo,
                                 int64_t sOc, int64_t sOg, int order, int reduce_cols, void* stream) {
    MmCall c{};
    c.dtype = dtype; c.A = A; c.B = B; c.sAc = sAc; c.sAg = sAg; c.sBc = sBc; c.sBg = sBg;
    c.M = M; c.N = N; c.Kp = Kp; c.k_valid = k_valid; c.C = C; c.G = G; c.gmod = gmod;
    c.ref = ref; c.ldr = ldr; c.sRg = sRg; c.ref_cs = ref_cs; c.ref_div = ref_div;
    c.sa = sa; c.sa_c = sa_c; c.sa_g = sa_g; c.sa_mul = sa_mul;
    c.sb = sb; c.sb_c = sb_c; c.sb_g = sb_g; c.sb_n = sb_n;
    c.bias = bias; c.bi_c = bi_c; c.bi_g = bi_g; c.bi_n = bi_n;
    c.row_scale = row_scale; c.row_bias = row_bias;
    c.partial = partial; c.partial_elems = partial_elems;
    c.out = out; c.ldo = ldo; c.sOc = sOc; c.sOg = sOg;
    c.order = order; c.reduce_cols = reduce_cols; c.stream = stream;
    return gemm_score_impl(c);
}

// quant_forward product from packed operands with the epilogue extras (reference quant_layers/linear.py:46-51, matmul.py:43-45,
// utils/wrap_net.py:30-31):  out[g][m][n] = sa[gh * sa_g] * sa_mul * sb[gh * sb_g + n * sb_n] * (A[g] . B[g]^T)[m][n]
//                                            + bias[gh * bi_g + n * bi_n] + addend[g][m][n]
// A [G][M][Kp], B [G][N][Kp] packed int8 (dtype 0) / bf16 (1) operands (group strides in elements; 0 = shared), gh = g % gmod.
// addend (may be null): the residual stream, indexed like out.  out_gi > 0: two-level output groups -- group g is written at
// (g % out_gi) * sOg + (g / out_gi) * sOo, e.g. softmax . v with out_gi = H, sOg = D, sOo = N * H * D, ldo = H * D writes
// [B][N][H][D] storage, so that the transpose(1, 2).reshape(B, N, C) in front of the projection layer is a view.
extern "C" int adalog_gemm_out_ex(int dtype, const void* A, const void* B, int64_t sAg, int64_t sBg, int M, int N, int64_t Kp, int G,
                                  int gmod, const float* sa, int64_t sa_g, float sa_mul, const float* sb, int64_t sb_g, int64_t sb_n,
                                  const float* bias, int64_t bi_g, int64_t bi_n, const float* addend, float* out, int64_t ldo,
                                  int64_t sOg, int out_gi, int64_t sOo, void* stream) {
    ADALOG_ARG_CHECK(out && (dtype == 0 || dtype == 1), "gemm_out_ex: int8 or bf16 operands, out required");
    const MmOutEx ox{addend, out_gi, sOo};
    MmCall c{};                                                       // no candidate axis, no reference: ref_cs = ref_div = 1
    c.dtype = dtype; c.A = A; c.B = B; c.sAg = sAg; c.sBg = sBg;
    c.M = M; c.N = N; c.Kp = Kp; c.C = 1; c.G = G; c.gmod = gmod; c.ref_cs = 1; c.ref_div = 1;
    c.sa = sa; c.sa_g = sa_g; c.sa_mul = sa_mul;
    c.sb = sb; c.sb_g = sb_g; c.sb_n = sb_n;
    c.bias = bias; c.bi_g = bi_g; c.bi_n = bi_n;
    c.out = out; c.ldo = ldo; c.sOg = sOg; c.stream = stream; c.ox = &ox;
    return gemm_score_impl(c);
}

// quant_forward of a uniformly quantised Linear layer / q.k^T product (reference quant_layers/linear.py:46-51, matmul.py:43-45) with
// the A-side fake quantisation INSIDE the GEMM's loader (k_gemm_cand<.., GENA>):
//   out[g][m][n] = sa[gh * sa_g] * sa_mul * sb[gh * sb_g + n * sb_n] * sum_k (q_a(x[g][m][k]) - z_a) * B[g][n][k] + bias[gh * bi_g + n * bi_n]
// x fp32 [G][M][ldx] (groups sxg apart, K valid, K % 16 == 0), (a_scale, a_zp)[gh * a_pg] its per-tensor (a_pg = 0) / per-head
// quantiser (gh = g % gmod), B the packed int8 operand [G][N][Kp] (adalog_pack_uniform).  Same result, bit for bit, as
// adalog_pack_uniform(x) + adalog_gemm_score(out): the activation is read once as fp32 instead of written and re-read as int8, and
// one launch per layer disappears.  adalog_gemm_out_gen below is the entry point; its relatives share gemm_out_gen_impl.

// The A side of adalog_gemm_out_gen and its relatives: the fp32 activation and its quantiser, the row maps (null = identity)
struct MmGenA { const float* x; int64_t ldx, sxg; int K; const float *a_scale, *a_zp; int64_t a_pg; int n_bits; const int *a_rows, *o_rows; int64_t period; };

// c: the store call (B, sizes, epilogue, out; addend in c.ox); g: where A comes from
static int gemm_out_gen_impl(const MmCall& c, const MmGenA& g) {
    const float *x = g.x, *a_scale = g.a_scale, *a_zp = g.a_zp, *addend = c.ox->addend;
    const int64_t ldx = g.ldx, Kp = c.Kp;
    const int K = g.K, n_bits = g.n_bits, M = c.M, N = c.N, G = c.G, gmod = c.gmod;
    const void* B = c.B;
    ADALOG_ARG_CHECK(x && a_scale && a_zp && B && c.sa && c.sb && c.out, "gemm_out_gen: null pointer");
    ADALOG_ARG_CHECK(M >= 1 && N >= 1 && G >= 1 && gmod >= 1 && G % gmod == 0 && K >= 16 && K % 16 == 0 && Kp >= K && Kp % BK2 == 0,
                     "gemm_out_gen: K must be a multiple of 16, Kp a multiple of 128 covering it");
    ADALOG_ARG_CHECK(n_bits >= 2 && n_bits <= 7 && ldx >= K && ldx % 4 == 0 && g.sxg % 4 == 0 && (((uintptr_t)x) & 15) == 0 &&
                     (((uintptr_t)B) & 15) == 0, "gemm_out_gen: <= 7-bit quantiser, 16-byte aligned fp32 rows");
    ADALOG_ARG_CHECK((int64_t)M * ldx < ((int64_t)1 << 31) && (int64_t)N * Kp < ((int64_t)1 << 31), "gemm_out_gen: operand exceeds 32-bit addressing");
    // 128-row tiles while they give every CU one, else 64-row tiles (attn.proj of deit_small: 50 x 2 -> 99 x 2 tiles)
    int tmv = pick_tm_out(M, (int64_t)cdiv(N, BN2) * G);
    if (tmv > 2) tmv = 2;
    Layout L{};
    L.MT = cdiv(M, 64 * tmv); L.NT = cdiv(N, BN2); L.Npad = L.NT * BN2;
    GemmArgs p = gemm_args(c, L);                                     // (c.k_valid = K: the valid bytes of the int8 rows)
    p.KbA = Kp; p.timeline = nullptr;                                 // the generated rows are as long as B's; never timed in the lab
    p.gen_x = x; p.gen_ldx = ldx; p.gen_sg = g.sxg; p.gen_K = K; p.gen_scale = a_scale; p.gen_zp = a_zp; p.gen_sn = g.a_pg;
    p.gen_qmax = (float)((1 << n_bits) - 1);
    const bool rowmap = g.a_rows || g.o_rows;
    p.a_rows = g.a_rows; p.o_rows = g.o_rows; p.row_period = (int)(rowmap ? g.period : 1);
    const int64_t tiles = (int64_t)p.MT * p.NT * G;
    ADALOG_ARG_CHECK(tiles < ((int64_t)1 << 31), "gemm_out_gen: grid too large");
    const size_t shm = (size_t)(64 * tmv + BN2) * BK2 + (512 + 256) * sizeof(float);
    const char* label = rowmap ? "k_gemm_cand_gen_rows" : addend ? "k_gemm_cand_gen_ex" : "k_gemm_cand_gen";
    if (const int e = adalog_dispatch<true, false>(rowmap, [&](auto map) {
            return adalog_dispatch<true, false>(addend != nullptr, [&](auto add) {
                return adalog_dispatch<2, 1>(tmv, [&](auto tm) {
                    return adalog_launch<k_gemm_cand<0, decltype(tm)::value, true, true, decltype(add)::value, decltype(map)::value>>(
                        label, 72 * 1024, (unsigned)tiles, 512, shm, (hipStream_t)c.stream, p);
                });
            });
        })) return e;
    ADALOG_LAUNCH_CHECK("adalog_gemm_out_gen");
    return 0;
}

// addend[g][m][n] (same strides as out; may be null): the residual stream added in the epilogue (x + proj(...) of a transformer block)
extern "C" int adalog_gemm_out_gen(const float* x, int64_t ldx, int64_t sxg, int K, const float* a_scale, const float* a_zp, int64_t a_pg,
                                   int n_bits, const void* B, int64_t sBg, int M, int N, int64_t Kp, int G, int gmod, const float* sa,
                                   int64_t sa_g, float sa_mul, const float* sb, int64_t sb_g, int64_t sb_n, const float* bias,
                                   int64_t bi_g, int64_t bi_n, const float* addend, float* out, int64_t ldo, int64_t sOg, void* stream) {
    const MmOutEx ox{addend, 0, 0};
    const MmGenA g{x, ldx, sxg, K, a_scale, a_zp, a_pg, n_bits, nullptr, nullptr, 1};
    MmCall c{};
    c.B = B; c.sBg = sBg; c.M = M; c.N = N; c.Kp = Kp; c.k_valid = K; c.C = 1; c.G = G; c.gmod = gmod; c.ref_cs = 1; c.ref_div = 1;
    c.sa = sa; c.sa_g = sa_g; c.sa_mul = sa_mul; c.sb = sb; c.sb_g = sb_g; c.sb_n = sb_n; c.bias = bias; c.bi_g = bi_g; c.bi_n = bi_n;
    c.out = out; c.ldo = ldo; c.sOg = sOg; c.stream = stream; c.ox = &ox;
    return gemm_out_gen_impl(c, g);
}

// ... with the rows of one group (G = 1) remapped in periods of L rows (the tokens of one image): A row r is read from x row
// a_rows[r % L] + (r / L) L, and out / addend row o_rows[r % L] + (r / L) L is written (either map may be null = identity; entries in
// [0, L); o_rows a permutation, so that every output row is written once).  Swin: a_rows = the roll + window partition in front of
// qkv, o_rows = the same map behind proj with the block input as addend.
extern "C" int adalog_gemm_out_gen_rows(const float* x, int64_t ldx, int K, const float* a_scale, const float* a_zp, int n_bits,
                                        const void* B, int M, int N, int64_t Kp, const float* sa, float sa_mul, const float* sb,
                                        int64_t sb_n, const float* bias, int64_t bi_n, const float* addend, float* out, int64_t ldo,
                                        const int* a_rows, const int* o_rows, int64_t period, void* stream) {
    ADALOG_ARG_CHECK(period >= 1 && M % period == 0, "gemm_out_gen_rows: M must be a multiple of the period");
    ADALOG_ARG_CHECK(ldo >= N && (int64_t)M * ldo < ((int64_t)1 << 31), "gemm_out_gen_rows: output exceeds 32-bit addressing");
    const MmOutEx ox{addend, 0, 0};
    const MmGenA g{x, ldx, 0, K, a_scale, a_zp, 0, n_bits, a_rows, o_rows, period};
    MmCall c{};                                                       // one group, per-tensor quantiser and factors
    c.B = B; c.M = M; c.N = N; c.Kp = Kp; c.k_valid = K; c.C = 1; c.G = 1; c.gmod = 1; c.ref_cs = 1; c.ref_div = 1;
    c.sa = sa; c.sa_mul = sa_mul; c.sb = sb; c.sb_n = sb_n; c.bias = bias; c.bi_n = bi_n;
    c.out = out; c.ldo = ldo; c.stream = stream; c.ox = &ox;
    return gemm_out_gen_impl(c, g);
}

// Attention searches with uniform candidates (reference quant_layers/matmul.py:135-163 / 173-201), GEN form: scores of the
// ref_div candidates (sb, zp)[c * sb_c + head * sb_g] of the operand x [G][N / ref_div][K = k_valid] (fp32, rows ldx apart, groups
// sg apart) against the packed fixed operand A [G][M][Kp] -- what adalog_gemm_score computes from the packed candidate operand
// [G][N][Kp] (candidates innermost), without that operand: the kernels quantise x in registers (k_gemm_win / k_gemm_grpw, GEN).
// Transposed reference (ref_cs = M), per-workgroup fp64 accumulators: the partial-buffer layout of adalog_gemm_score_layout.
// Shapes: adalog_gemm_score_gen_ok.
extern "C" int adalog_gemm_score_gen(int dtype, const void* A, int64_t sAg, int M, int N, int64_t Kp, int64_t k_valid, int G, int gmod,
                                     const float* x, int64_t ldx, int64_t sg, const float* zp, int n_bits, const float* ref,
                                     int64_t sRg, int ref_div, const float* sa, int64_t sa_c, int64_t sa_g, float sa_mul,
                                     const float* sb, int64_t sb_c, int64_t sb_g, float* partial, int64_t partial_elems,
                                     void* stream) {
    ADALOG_ARG_CHECK(n_bits >= 1 && n_bits <= 8 && (dtype != 3 || n_bits <= 4), "gemm_score_gen: fp8 candidates hold <= 4-bit values");
    const MmGen gen{x, ldx, sg, zp, n_bits};
    MmCall c{};                                                       // no B, no bias; transposed reference, per-workgroup sums
    c.dtype = dtype; c.A = A; c.sAg = sAg; c.M = M; c.N = N; c.Kp = Kp; c.k_valid = k_valid; c.C = 1; c.G = G; c.gmod = gmod;
    c.ref = ref; c.ldr = 1; c.sRg = sRg; c.ref_cs = M; c.ref_div = ref_div;
    c.sa = sa; c.sa_c = sa_c; c.sa_g = sa_g; c.sa_mul = sa_mul; c.sb = sb; c.sb_c = sb_c; c.sb_g = sb_g;
    c.partial = partial; c.partial_elems = partial_elems; c.order = 2; c.reduce_cols = 1; c.stream = stream; c.gen = &gen;
    return gemm_score_impl(c);
}

// ---- softmax.v searches with the candidate operand GENERATED inside the kernel (adalog_gemm_score_avq / _avw): what they share.
// The Layout both are planned on -- the bf16 launch of the shape with P candidates per reference column
static Layout av_layout(int M, int N, int G, int gmod, int P, int64_t k_valid, int64_t Kp) {
    return layout_of(M, N * P, 1, G, gmod, P, 1, true, k_valid * 2, Kp * 2, true, 1);
}
// ... and the kernel arguments they share: C = 1, bf16 rows of A, transposed reference, column factors without a column stride,
// per-workgroup fp64 accumulators, B generated from x [G][N][K].  Each entry point states its row lengths, its quantiser and its items
// after this fill.
static GemmArgs av_gen_args(const void* A, int64_t sAg, int M, int N, int64_t k_valid, int G, int gmod, const float* x, int64_t ldx,
                            int64_t sg, const float* ref, int64_t sRg, int P, const float* sa, int64_t sa_c, int64_t sa_g, float sa_mul,
                            const float* sb, int64_t sb_c, int64_t sb_g, float* partial) {
    GemmArgs p{};
    p.A = (const uint8_t*)A; p.sAg = sAg * 2; p.M = M; p.N = N * P; p.C = 1; p.G = G; p.gmod = gmod;
    p.ref = ref; p.ldr = 1; p.sRg = sRg; p.ref_cs = M; p.ref_div = P;
    p.sa = sa; p.sa_c = sa_c; p.sa_g = sa_g; p.sa_mul = sa_mul; p.sb = sb; p.sb_c = sb_c; p.sb_g = sb_g;
    p.wg_acc = (double*)partial; p.partial = partial; p.gen_x = x; p.gen_ldx = ldx; p.gen_sg = sg; p.gen_K = (int)k_valid;
    return p;
}

// softmax.v, log-base search of the post-softmax AdaLog quantiser (reference quant_layers/matmul.py:321-351): scores of the P = 128
// candidate bases q against the reference, with the candidate operand (P AdaLog quantisations of the probabilities x [G][N][K]:
// scale 1, no clamp) generated inside the kernel (k_gemm_avq) instead of packed by adalog_pack_adalog_bf16 and streamed.
//   A: the fixed operand v^T, bf16 [G][M <= 64][Kp] (K-contiguous, zero past K);  q: the bases [P];
//   lut: dword table [2^n_bits + 1][P], entry [k][c] = bf16 bits of the value of bin k under base q[c] (numerator * 2^-t, what
//        the packer writes), row 2^n_bits = 0 (the masked code);  ref [G][N][M];  sa / sb / sa_mul / partial as adalog_gemm_score
//        (C = 1, ref_div = P, reduce_cols = 1: the per-workgroup fp64 accumulators of adalog_gemm_score_layout with dtype 1).
// (L: where the launch's Layout goes, for the call)
static bool avq_ok(int M, int N, int G, int gmod, int P, int64_t k_valid, int64_t Kp, int n_bits, Layout* L = nullptr) {
    static const int use_avq = getenv("ADALOG_GEMM_AVQ") ? atoi(getenv("ADALOG_GEMM_AVQ")) : 1;
    if (!use_avq || P != 128 || M < 1 || M > 64 || N < 1 || k_valid < 1 || k_valid > 208 || n_bits < 1 || n_bits > 6 || gmod < 1 || gmod > 16 ||
        G % gmod || G < 8)
        return false;
    const int nks = k_valid <= 64 ? 4 : 13;
    if (Kp < nks * 16 || (Kp * 2) % 16) return false;
    const Layout l = av_layout(M, N, G, gmod, P, k_valid, Kp);
    if (L) *L = l;
    return l.stream && l.acc && !l.slab && l.wgs * 4 >= gmod;
}
extern "C" int adalog_gemm_score_avq_ok(int M, int N, int G, int gmod, int P, int64_t k_valid, int64_t Kp, int n_bits) {
    return avq_ok(M, N, G, gmod, P, k_valid, Kp, n_bits) ? 1 : 0;
}
extern "C" int adalog_gemm_score_avq(const void* A, int64_t sAg, int M, int N, int64_t Kp, int64_t k_valid, int G, int gmod,
                                     const float* x, int64_t ldx, int64_t sg, const float* q, const uint32_t* lut, int n_bits,
                                     const float* ref, int64_t sRg, int P, const float* sa, int64_t sa_c, int64_t sa_g, float sa_mul,
                                     const float* sb, int64_t sb_c, int64_t sb_g, float* partial, int64_t partial_elems,
                                     void* stream) {
    ADALOG_ARG_CHECK(A && x && q && lut && ref && sa && sb && partial, "gemm_score_avq: null pointer");
    Layout L{};
    ADALOG_ARG_CHECK(avq_ok(M, N, G, gmod, P, k_valid, Kp, n_bits, &L), "gemm_score_avq: shape not taken (adalog_gemm_score_avq_ok)");
    ADALOG_ARG_CHECK((((uintptr_t)A) & 15) == 0 && (((uintptr_t)partial) & 7) == 0, "gemm_score_avq: operand / accumulator alignment");
    ADALOG_ARG_CHECK(partial_elems >= L.elems, "gemm_score_avq: partial buffer too small");
    GemmArgs p = av_gen_args(A, sAg, M, N, k_valid, G, gmod, x, ldx, sg, ref, sRg, P, sa, sa_c, sa_g, sa_mul, sb, sb_c, sb_g, partial);
    p.Kb = Kp * 2; p.Kvb = k_valid * 2; p.gen_q = q; p.gen_lut = lut; p.gen_nb = 1 << n_bits;
    wave_chunks(p, N, L.wgs, G, cdiv(N, AVQ_ROWS));                 // <= AVQ_ROWS attention rows per item (they are staged in LDS)
    const int nks = k_valid <= 64 ? 4 : 13;
    const size_t lut_b = (((size_t)(p.gen_nb + 1) * P + 3) & ~(size_t)3) * 4;
    const size_t rows_b = (size_t)4 * ((size_t)AVQ_ROWS * (nks * 16 + 64) + 4 * 64 * 2) * 4;
    const size_t acc_b = (size_t)gmod * 256 * 8;
    const size_t shm = lut_b + rows_b > acc_b ? lut_b + rows_b : acc_b;
    hipStream_t st = (hipStream_t)stream;
    const unsigned wgs = (unsigned)L.wgs;
    const int e = nks == 13 ? (M > 32 ? adalog_launch<k_gemm_avq<4, 13, 2>>("k_gemm_avq<13,bf16>", 80 * 1024, wgs, 256, shm, st, p)
                                      : adalog_launch<k_gemm_avq<4, 13, 1>>("k_gemm_avq<13,bf16>", 80 * 1024, wgs, 256, shm, st, p))
                            : (M > 32 ? adalog_launch<k_gemm_avq<4, 4, 2>>("k_gemm_avq<4,bf16>", 80 * 1024, wgs, 256, shm, st, p)
                                      : adalog_launch<k_gemm_avq<4, 4, 1>>("k_gemm_avq<4,bf16>", 80 * 1024, wgs, 256, shm, st, p));
    if (e) return e;
    ADALOG_LAUNCH_CHECK("adalog_gemm_score_avq");
    return 0;
}

// softmax.v, search over the uniform quantiser of v (reference quant_layers/matmul.py:173-201): the launch of adalog_gemm_score with
// dtype 4 (bf16 rows x fp8 candidate columns, trimmed K: k_gemm_grpk8t) without its packed candidate operand -- the P quantisations
// of v^T x [G][N][K] (fp32, rows ldx, groups sg apart) are generated inside the kernel (k_gemm_avw_gen) from the candidates' scales
// (sb, the epilogue's column factors) and zero points (zp, same indexing).  Same items on the same grid, same MFMA and reduction
// order: the partials equal those of the packed launch bit for bit wherever that launch exists.
//   A: the fixed operand, packed bf16 [G][M <= 224][Kp] (zero past K; Kp a multiple of 8); K <= 200 (13 MFMAs); N a multiple of 32;
//   P = 64, 128 or 256 candidates of <= 4 bits; partial: per-workgroup fp64 accumulators [workgroups][gmod][256].
// adalog_gemm_score_avw_ok: 0 when the shape is not taken, otherwise the number of workgroups (the partial buffer's leading extent).
// The kernel is built for k_gemm_grpk8t's family (193 .. 200 keys, 129 .. 224 rows): a block always costs 13 MFMAs and an item the
// load of the whole LDS image (M <= 224: at most 90 064 bytes), so shorter K or fewer rows are computed correctly but wastefully.  The
// predicate takes them (the tests run them); the search asks for this form only above 64 keys, where it ran k_gemm_grpk8t --
// windows (K <= 64) stay on k_gemm_winb.
static int avw_wgs(int M, int N, int G, int gmod, int P, int64_t k_valid, int64_t Kp, int n_bits) {
    if (!(P == 64 || P == 128 || P == 256) || M < 1 || M > 224 || N < 32 || N % 32 || k_valid < 1 || k_valid > 200 || Kp < k_valid || Kp % 8 ||
        n_bits < 1 || n_bits > 4 || gmod < 1 || G < 1 || G % gmod || (int64_t)N * P >= ((int64_t)1 << 30))
        return 0;
    const Layout L = av_layout(M, N, G, gmod, P, k_valid, Kp);
    return (L.stream && L.acc && !L.slab && L.wgs >= 1) ? L.wgs : 0;
}
extern "C" int adalog_gemm_score_avw_ok(int M, int N, int G, int gmod, int P, int64_t k_valid, int64_t Kp, int n_bits) {
    return avw_wgs(M, N, G, gmod, P, k_valid, Kp, n_bits);
}
extern "C" int adalog_gemm_score_avw(const void* A, int64_t sAg, int M, int N, int64_t Kp, int64_t k_valid, int G, int gmod,
                                     const float* x, int64_t ldx, int64_t sg, const float* zp, int n_bits, const float* ref, int64_t sRg,
                                     int P, const float* sa, int64_t sa_c, int64_t sa_g, float sa_mul, const float* sb, int64_t sb_c,
                                     int64_t sb_g, float* partial, int64_t partial_elems, void* stream) {
    ADALOG_ARG_CHECK(A && x && zp && ref && sa && sb && partial, "gemm_score_avw: null pointer");
    const int wgs = avw_wgs(M, N, G, gmod, P, k_valid, Kp, n_bits);
    ADALOG_ARG_CHECK(wgs > 0, "gemm_score_avw: shape not taken (adalog_gemm_score_avw_ok)");
    ADALOG_ARG_CHECK((((uintptr_t)A) & 15) == 0 && (sAg * 2) % 16 == 0 && (((uintptr_t)partial) & 7) == 0 && (((uintptr_t)x) & 3) == 0,
                     "gemm_score_avw: operand / accumulator alignment");
    ADALOG_ARG_CHECK(ldx >= k_valid && (int64_t)N * ldx * 4 < ((int64_t)1 << 31), "gemm_score_avw: rows of x shorter than K, or a group of x beyond 32-bit addressing");
    ADALOG_ARG_CHECK(partial_elems >= (int64_t)2 * wgs * gmod * BN2, "gemm_score_avw: partial buffer too small");
    GemmArgs p = av_gen_args(A, sAg, M, N, k_valid, G, gmod, x, ldx, sg, ref, sRg, P, sa, sa_c, sa_g, sa_mul, sb, sb_c, sb_g, partial);
    p.Kb = Kp; p.KbA = Kp * 2; p.Kvb = k_valid; p.gen_zp = zp; p.gen_qmax = (float)((1 << n_bits) - 1);
    grp_chunks(p, N * P, wgs, G);                                  // k_gemm_grpk8t's items
    const size_t shm = (size_t)avw_lds_bytes(M);              // [M + 1 rows][25 slots], a zero tail, the reference column(s)
    hipStream_t st = (hipStream_t)stream;
    if (const int e = with_nj(P, [&](auto nj) {
            constexpr int NJ = decltype(nj)::value;
            return M > 192 ? adalog_launch<k_gemm_avw_gen<NJ, true>>("k_gemm_avw_gen<13,bf16>", 160 * 1024, (unsigned)wgs, NJ * 64, shm, st, p)
                           : adalog_launch<k_gemm_avw_gen<NJ, false>>("k_gemm_avw_gen<13,bf16>", 160 * 1024, (unsigned)wgs, NJ * 64, shm, st, p);
        })) return e;
    ADALOG_LAUNCH_CHECK("adalog_gemm_score_avw");
    return 0;
}

// 1 when adalog_gemm_score_gen takes this shape (M rows of the fixed operand, N = source rows x ref_div candidate columns).
extern "C" int adalog_gemm_score_gen_ok(int dtype, int M, int N, int G, int gmod, int ref_div, int64_t k_valid, int64_t Kp) {
    if (!(dtype == 0 || dtype == 3) || k_valid < 16 || k_valid > 64 || k_valid % 16 || ref_div < 1 || N % ref_div != 0 || G % gmod) return 0;
    const MmCall c = shape_call(dtype, M, N, G, gmod, ref_div, k_valid, Kp, 1);
    const Route r = route_of(c, call_layout(c, true));
    return (r == R_WIN || r == R_GRPW) ? 1 : 0;
}

// ---- the two scoring calls with the candidate operand GENERATED inside the slab kernel (k_gemm_slab<.., GEN>): what they share.
// One group, the packed fixed operand A [rows][Kp] against cols x P columns generated from x [cols][ldx] (K valid) with the
// candidates (scale, zp), transposed reference [cols][rows], the slab items of the Layout.  Each entry point states its epilogue
// factors and the candidates' strides (sa / sb_c / sb_n / row_* / bias / gen_sc / gen_sn / gen_sa) after this fill.
static GemmArgs slab_gen_args(const Layout& L, const void* A, int rows, int64_t cols, int64_t Kp, const float* x, int64_t ldx, int K,
                              const float* scale, const float* zp, int P, int n_bits, const float* ref, float* partial) {
    GemmArgs p{};
    p.A = (const uint8_t*)A; p.M = rows; p.N = (int)(cols * P); p.Kb = Kp; p.Kvb = K; p.C = 1; p.G = 1; p.gmod = 1;
    p.ref = ref; p.ldr = 1; p.ref_cs = rows; p.ref_div = P; p.sa_mul = 1.0f; p.sb = scale;
    p.MT = L.MT; p.NT = L.NT; p.Npad = L.Npad; p.order = 2; p.reduce_cols = 0; p.timeline = g_timeline;
    p.partial = partial; p.slab_U = L.slab_U; p.slab_R = L.slab_R;
    p.gen_x = x; p.gen_ldx = ldx; p.gen_K = K; p.gen_scale = scale; p.gen_zp = zp; p.gen_qmax = (float)((1 << n_bits) - 1);
    // tie zone: the reciprocal-multiply quotient is within ~2 ulp of the IEEE one; only |quotient| <= 2^bits matters (beyond it
    // both clamp alike), so 6e-7 * 2^bits bounds the difference with a factor of 2.5 to spare; never narrower than 1e-5
    const float zone = 6e-7f * (float)(1 << n_bits);
    p.gen_tie = 0.5f - (zone > 1e-5f ? zone : 1e-5f);
    return p;
}
// ... and their launch.  SCORE_ACT: the kernel's second template argument (per-row factors: the activation search); form: slab_label's
template <bool SCORE_ACT>
static int slab_gen_launch(int form, int dtype, const Layout& L, int P, hipStream_t st, const GemmArgs& p) {
    const size_t shm = slab_lds(p.Kvb, L.slab_nb);
    return with_slab(dtype, L.slab_nb, P, [&](auto nr, auto dt, auto nb) {
        constexpr int NREF = decltype(nr)::value, DT = decltype(dt)::value, NB = decltype(nb)::value;
        return adalog_launch<k_gemm_slab<NREF, SCORE_ACT, DT, NB, true>>(slab_label(form, DT, NB), 160 * 1024, (unsigned)L.wgs, 512, shm, st, p);
    });
}

// ---- activation-candidate scoring call with the candidate operand GENERATED inside the slab kernel (k_gemm_slab<.., GEN>)
// reference linear.py:394-430 (_search_best_a_scale): scores[p] = -norm * sum_{t, o} (raw_out[t][o] - bias[o] -
//   s_w[o] * s_p * sum_k Wq[o][k] * (clamp(rne(x[t][k] / s_p) + z_p, 0, 2^bits - 1) - z_p))^2
// Wp: packed weight image (q_w - z_w) [M][Kp] int8 (dtype 0) or fp8 e4m3 (dtype 3); x: fp32 [T][ldx] (K valid); ref: raw_out
// [T][M]; scale / zp: the P (64, 128 or 256) per-tensor candidates; row_scale [M] = s_w, row_bias [M] = bias (or null).
static Layout gen_layout(int dtype, int M, int64_t T, int K, int64_t Kp, int P) {
    Layout L{};
    if (!(dtype == 0 || dtype == 3) || !(P == 64 || P == 128 || P == 256) || T < 1 || T * P >= ((int64_t)1 << 31) || K < 16 || K % 16 != 0 ||
        Kp < K) return L;
    return layout_of(M, (int)(T * P), 1, 1, 1, P, 1, true, (int64_t)K, Kp, true, dtype, true);
}

extern "C" int adalog_score_act_gen_ok(int dtype, int M, int64_t T, int K, int64_t Kp, int P) {
    static const int use_gen = getenv("ADALOG_SLAB_GEN") ? atoi(getenv("ADALOG_SLAB_GEN")) : 1;
    if (!use_gen || Kp % BK3 != 0) return 0;
    const Layout L = gen_layout(dtype, M, T, K, Kp, P);
    return (L.slab && L.acc) ? 1 : 0;
}

extern "C" int adalog_score_act_gen_wgs(int dtype, int M, int64_t T, int K, int64_t Kp, int P) {
    const Layout L = gen_layout(dtype, M, T, K, Kp, P);
    return (L.slab && L.acc) ? L.wgs : -1;
}

extern "C" int64_t adalog_score_act_gen_workspace_bytes(int dtype, int M, int64_t T, int K, int64_t Kp, int P) {
    const Layout L = gen_layout(dtype, M, T, K, Kp, P);
    if (!(L.slab && L.acc)) return -1;
    return L.elems * (int64_t)sizeof(float) + ((int64_t)M * 4 + 15) / 16 * 16;          // accumulators + a zero row-bias vector
}

extern "C" int adalog_score_act_gen(int dtype, const void* Wp, int M, int64_t Kp, const float* x, int64_t T, int K, int64_t ldx,
                                    const float* scale, const float* zp, int P, int n_bits, const float* ref,
                                    const float* row_scale, const float* row_bias, double norm, void* workspace,
                                    int64_t workspace_bytes, float* scores, void* stream) {
    ADALOG_ARG_CHECK(Wp && x && scale && zp && ref && row_scale && workspace, "score_act_gen: null pointer");
    ADALOG_ARG_CHECK(n_bits >= 2 && n_bits <= 7 && (dtype != 3 || n_bits <= 4), "score_act_gen: bad bit width for the operand type");
    ADALOG_ARG_CHECK(ldx >= K && (ldx % 4 == 0) && ((uintptr_t)x & 15) == 0, "score_act_gen: activation rows must be 16-byte aligned");
    const Layout L = gen_layout(dtype, M, T, K, Kp, P);
    ADALOG_ARG_CHECK(L.slab && L.acc && Kp % BK3 == 0, "score_act_gen: shape not taken by the slab kernel (adalog_score_act_gen_ok)");
    ADALOG_ARG_CHECK(workspace_bytes >= adalog_score_act_gen_workspace_bytes(dtype, M, T, K, Kp, P) && ((uintptr_t)workspace & 15) == 0,
                     "score_act_gen: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)workspace;
    float* zero_bias = (float*)((uint8_t*)workspace + L.elems * sizeof(float));
    if (!row_bias) {
        const hipError_t me = hipMemsetAsync(zero_bias, 0, (size_t)M * 4, st);
        if (me != hipSuccess) { adalog_set_error("adalog_score_act_gen (zero bias)", me); return (int)me; }
        row_bias = zero_bias;
    }
    GemmArgs p = slab_gen_args(L, Wp, M, T, Kp, x, ldx, K, scale, zp, P, n_bits, ref, partial);
    ADALOG_ARG_CHECK((int64_t)(T - 1) * M + M < ((int64_t)1 << 31), "score_act_gen: reference exceeds 32-bit addressing");
    p.sa = scale; p.sb_c = 1; p.row_scale = row_scale; p.row_bias = row_bias; p.wg_acc = (double*)partial; p.gen_sc = 1;
    if (const int e = slab_gen_launch<true>(1, dtype, L, P, st, p)) return e;
    ADALOG_LAUNCH_CHECK("adalog_score_act_gen");
    // fixed-order fp64 finish of the per-workgroup accumulators [wgs][1][256] (scores == null: left to the caller, who hands the
    // accumulators -- the start of the workspace -- to adalog_finish_scores / adalog_finish_topk_next with MT = adalog_score_act_gen_wgs)
    if (!scores) return 0;
    return adalog_finish_scores(partial, scores, L.wgs, BN2, BN2, P, 1, 1, 0, 0, 2, norm, nullptr, 0, stream);
}

// ---- weight-candidate scoring call with the candidate operand GENERATED inside the slab kernel
// reference linear.py:355-392 (_search_best_w_scale): score[p][o] = -norm * sum_t (raw_out[t][o] - bias[o] -
//   s_a * s_w[p][o] * sum_k (q_a(x) - z_a)[t][k] * (clamp(rne(W[o][k] / s_w[p][o]) + z_w[p][o], 0, 2^bits - 1) - z_w[p][o]))^2
// Xp: packed activation image (q_a - z_a) [T][Kp] int8 (dtype 0) or fp8 e4m3 (dtype 3); W: fp32 [O][ldw] (K valid); scale / zp:
// the P (64, 128 or 256) candidates of every output row, [P][O]; ref: raw_out TRANSPOSED [O][T]; sa: device scalar s_a; bias [O]
// or null.  The packed [O * P][Kp] candidate operand (56-117 MB per call) is neither written nor read.  partial: the layout of
// adalog_gemm_score_layout(T, O * P, 1, 1, 1, P, 0, dtype, Kp, K, 1) (per-column partial sums, kept axis = (o, p)).
static Layout wgen_layout(int dtype, int T, int O, int K, int64_t Kp, int P) {
    Layout L{};
    if (!(dtype == 0 || dtype == 3) || !(P == 64 || P == 128 || P == 256) || O < 1 || (int64_t)O * P >= ((int64_t)1 << 31) || K < 16 || K % 16 != 0 ||
        Kp < K) return L;
    return layout_of(T, O * P, 1, 1, 1, P, 0, true, (int64_t)K, Kp, true, dtype, false);
}

extern "C" int adalog_score_w_gen_ok(int dtype, int T, int O, int K, int64_t Kp, int P) {
    static const int use_gen = getenv("ADALOG_SLAB_WGEN") ? atoi(getenv("ADALOG_SLAB_WGEN")) : 1;
    if (!use_gen || Kp % BK3 != 0) return 0;
    const Layout L = wgen_layout(dtype, T, O, K, Kp, P);
    return (L.slab && !L.acc) ? 1 : 0;
}

extern "C" int adalog_score_w_gen(int dtype, const void* Xp, int T, int64_t Kp, const float* W, int O, int K, int64_t ldw,
                                  const float* scale, const float* zp, int P, int n_bits, const float* ref, const float* sa,
                                  const float* bias, float* partial, int64_t partial_elems, void* stream) {
    ADALOG_ARG_CHECK(Xp && W && scale && zp && ref && sa && partial, "score_w_gen: null pointer");
    ADALOG_ARG_CHECK(n_bits >= 2 && n_bits <= 7 && (dtype != 3 || n_bits <= 4), "score_w_gen: bad bit width for the operand type");
    ADALOG_ARG_CHECK(ldw >= K && (ldw % 4 == 0) && ((uintptr_t)W & 15) == 0, "score_w_gen: weight rows must be 16-byte aligned");
    const Layout L = wgen_layout(dtype, T, O, K, Kp, P);
    ADALOG_ARG_CHECK(L.slab && !L.acc && Kp % BK3 == 0, "score_w_gen: shape not taken by the slab kernel (adalog_score_w_gen_ok)");
    ADALOG_ARG_CHECK(partial_elems >= L.elems, "score_w_gen: partial buffer too small");
    hipStream_t st = (hipStream_t)stream;
    GemmArgs p = slab_gen_args(L, Xp, T, O, Kp, W, ldw, K, scale, zp, P, n_bits, ref, partial);
    ADALOG_ARG_CHECK((int64_t)(O - 1) * T + T < ((int64_t)1 << 31), "score_w_gen: reference exceeds 32-bit addressing");
    p.sa = sa; p.sb_c = O; p.sb_n = 1; p.bias = bias; p.bi_n = 1; p.gen_sc = O; p.gen_sn = 1; p.gen_sa = sa;
    {   // a slab that is not cut has unused pieces: they must read as zero
        const hipError_t me = hipMemsetAsync(partial, 0, (size_t)L.elems * sizeof(float), st);
        if (me != hipSuccess) { adalog_set_error("adalog_score_w_gen (clear partials)", me); return (int)me; }
    }
    if (const int e = slab_gen_launch<false>(2, dtype, L, P, st, p)) return e;
    ADALOG_LAUNCH_CHECK("adalog_score_w_gen");
    return 0;
}

// scores[c][h?][n?] = -norm * sum over (image, [h], m_tile, [n]) of partial[c][g][m_tile][n] with the layout returned by
// adalog_gemm_score_layout (MT, Npad); N = number of valid entries along the last axis (n_eff, or NT when reduced).
extern "C" int64_t adalog_finish_workspace_bytes(int MT, int N, int C, int G, int keep_n, int cand_inner) {
    if (cand_inner != 1 || keep_n || !(C == 64 || C == 128 || C == 256)) return 0;
    return (int64_t)G * MT * cdiv(N, FSEG) * C * (int64_t)sizeof(double);
}

extern "C" int adalog_finish_scores(const float* partial, float* scores, int MT, int N, int Npad, int C, int G, int gmod,
                                    int keep_h, int keep_n, int cand_inner, double norm, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
    ADALOG_ARG_CHECK(partial && scores && MT >= 1 && N >= 1 && Npad >= N && C >= 1 && G >= 1 && gmod >= 1 && G % gmod == 0,
                     "finish_scores: bad arguments");
    FinishArgs p{};
    p.partial = partial; p.scores = scores; p.C = C; p.G = G; p.gmod = gmod; p.MT = MT; p.N = N; p.Npad = Npad;
    p.keep_h = keep_h; p.keep_n = keep_n; p.norm = norm; p.cin = cand_inner ? C : 0;
    if (cand_inner == 2) {                  // per-workgroup accumulators: partial = double [MT = workgroups][gmod][256]
        ADALOG_ARG_CHECK(!keep_n && (C == 64 || C == 128 || C == 256) && Npad == 256, "finish_scores: bad accumulator layout");
        const int64_t nout2 = (int64_t)C * (keep_h ? gmod : 1);
        hipLaunchKernelGGL(k_finish_wgacc, dim3((unsigned)nout2), dim3(256), 0, (hipStream_t)stream, p,
                           (const double*)partial, MT);
        ADALOG_LAUNCH_CHECK("adalog_finish_scores");
        return 0;
    }
    const int64_t nout = (int64_t)C * (keep_h ? gmod : 1) * (keep_n ? N : 1);
    const int64_t per_out = (int64_t)(G / gmod) * (keep_h ? 1 : gmod) * MT * (keep_n ? 1 : N);
    const int64_t need = adalog_finish_workspace_bytes(MT, N, C, G, keep_n, cand_inner);
    if (need > 0 && workspace && workspace_bytes >= need && per_out >= 1024) {
        const int nseg = cdiv(N, FSEG);
        hipLaunchKernelGGL(k_finish_rows, dim3((unsigned)nseg, (unsigned)(G * MT)), dim3(256), 0, (hipStream_t)stream, p,
                           (double*)workspace, nseg);
        hipLaunchKernelGGL(k_finish_stage2, dim3((unsigned)((nout + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p,
                           (const double*)workspace, nseg);
    } else if (p.cin > 0 && per_out <= 512 && nout >= 4096)
        hipLaunchKernelGGL(k_finish_tpo, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    else if (per_out >= 2048)
        hipLaunchKernelGGL(k_finish<false>, dim3((unsigned)nout), dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(k_finish<true>, dim3((unsigned)((nout + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    ADALOG_LAUNCH_CHECK("adalog_finish_scores");
    return 0;
}

// finish + top-k + next grid in one launch where the layout allows it (see gemm_finish.inc); otherwise adalog_finish_scores
// followed by adalog_topk_next.  Arguments: those of adalog_finish_scores, then those of adalog_topk_next (scores [C][cols],
// cols = (keep_h ? gmod : 1) * (keep_n ? N : 1)).  Single-GPU only: with several ranks the scores are all-reduced between the two.
extern "C" int adalog_finish_topk_next_tail(const float* partial, float* scores, int MT, int N, int Npad, int C, int G, int gmod,
                                            int keep_h, int keep_n, int cand_inner, double norm, void* workspace, int64_t workspace_bytes,
                                            const adalog_fpcs_tail* tail, void* stream) {
    ADALOG_ARG_CHECK(partial && scores && tail && MT >= 1 && N >= 1 && Npad >= N && C >= 1 && C <= 256 && G >= 1 &&
                     gmod >= 1 && G % gmod == 0, "finish_topk_next: bad arguments");
    const char* why = fpcs::tail_problem(tail, C);
    ADALOG_ARG_CHECK(why == nullptr, why);
    static const int use_fused = getenv("ADALOG_FINISH_TOPK") ? atoi(getenv("ADALOG_FINISH_TOPK")) : 1;
    const int nh = keep_h ? gmod : 1, nn = keep_n ? N : 1, cols = nh * nn;
    FinishArgs p{};
    p.partial = partial; p.scores = scores; p.C = C; p.G = G; p.gmod = gmod; p.MT = MT; p.N = N; p.Npad = Npad;
    p.keep_h = keep_h; p.keep_n = keep_n; p.norm = norm; p.cin = cand_inner ? C : 0;
    const TopkArgs t = *tail;
    hipStream_t st = (hipStream_t)stream;
    const bool c_ok = (C == 64 || C == 128 || C == 256);
    if (use_fused && cand_inner == 2 && !keep_n && c_ok && Npad == 256 && nh <= 64) {
        unsigned int* ticket = adalog_ticket_slots_on(nh, stream);
        if (ticket) {
            hipLaunchKernelGGL(k_finish_wgacc_topk, dim3((unsigned)(C * nh)), dim3(256), 0, st, p, (const double*)partial, MT, t, ticket);
            ADALOG_LAUNCH_CHECK("adalog_finish_topk_next");
            return 0;
        }
    }
    const int64_t nout = (int64_t)C * cols;
    const int64_t per_out = (int64_t)(G / gmod) * (keep_h ? 1 : gmod) * MT * (keep_n ? 1 : N);
    if (use_fused && cand_inner == 1 && c_ok && per_out <= 512 && nout >= 4096) {
        const int gpb = 256 / C;
        hipLaunchKernelGGL(k_finish_tpo_topk, dim3((unsigned)((cols + gpb - 1) / gpb)), dim3(256), 0, st, p, t);
        ADALOG_LAUNCH_CHECK("adalog_finish_topk_next");
        return 0;
    }
    const int rc = adalog_finish_scores(partial, scores, MT, N, Npad, C, G, gmod, keep_h, keep_n, cand_inner, norm, workspace,
                                        workspace_bytes, stream);
    if (rc) return rc;
    return adalog_topk_next_tail(scores, C, cols, tail, nullptr, stream);
}

extern "C" int adalog_finish_topk_next(const float* partial, float* scores, int MT, int N, int Npad, int C, int G, int gmod,
                                       int keep_h, int keep_n, int cand_inner, double norm, void* workspace, int64_t workspace_bytes,
                                       int k, const float* scale, const float* zp, const float* third, int new_cnt,
                                       const float* lin, float* delta, int has_clamp, float clamp_min, float* out_scale,
                                       float* out_zp, float* out_third, void* stream) {
    const adalog_fpcs_tail t{k, new_cnt, has_clamp, clamp_min, scale, zp, third, lin, delta, delta, out_scale, out_zp, out_third};
    return adalog_finish_topk_next_tail(partial, scores, MT, N, Npad, C, G, gmod, keep_h, keep_n, cand_inner, norm, workspace,
                                        workspace_bytes, &t, stream);
}
