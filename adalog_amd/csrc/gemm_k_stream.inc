// Part of gemm_score.hip (one translation unit, included inside its anonymous namespace): persistent streaming kernel (candidate columns, counted-vmcnt LDS-DMA ring).
// ------------------------------------------------------------------------------------------------ streaming kernel
// Third-generation scoring kernel (every search: candidates in the column axis, reference rows contiguous).
// What the per-workgroup cycle stamps of tools/lab/gemm_lab.hip showed for the kernel above at K = 384 (three 128-byte
// steps per tile): of 14.2k cycles per tile only 3.1k were matrix work -- 1.6k set-up (index divisions, 64-bit address
// arithmetic), 1.7-3.2k waiting for the first stage, 4.8k main loop (every wave issues its six DMA requests back to
// back at the top of a step while the matrix pipe idles), 4.0-5.4k epilogue (six VALU per output), 2k barriers/stores,
// and nothing overlaps anything because one 147 KiB workgroup owns the CU.  Hence:
//   * PERSISTENT workgroups: each walks a strided list of tiles and its LDS-DMA ring (3 stages of 64-byte K-steps)
//     keeps streaming across tile boundaries, so set-up and first-stage latency are paid once per launch, not per tile;
//   * 256 threads, (64*TM) x 256 tile, wave tile (32*TM) x 128 (fewer ds_reads per MFMA), 77 KiB of LDS: TWO workgroups
//     per CU, un-synchronised, so one's epilogue (VALU) runs under the other's main loop (MFMA);
//   * buffer_load ... lds with a per-tile resource: one VGPR offset per request, k offset in an SGPR, and the requests
//     are issued between the MFMAs of a step instead of in front of them;
//   * epilogue on packed fp32 math: reference slice minus row/column bias, row scale and column factors are staged in
//     LDS during the tile's first K-step; per pair of outputs 2 cvt + 2..4 v_pk_* instead of 12 scalar VALU.
constexpr int BK3 = 64;
// tools/lab builds this file with GEMM_LAB_NO_DMA / GEMM_LAB_NO_MFMA to time the two halves of the main loop separately
#if defined(GEMM_LAB_NO_DMA)
#define STREAM_DMA(rsrc, dst, voff, soff) do { } while (0)
#else
#define STREAM_DMA(rsrc, dst, voff, soff) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (las_ptr)(dst), 16, voff, soff, 0, 0)
#endif
#define STREAM_DMA4(rsrc, dst, voff) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (las_ptr)(dst), 4, (int)(voff), 0, 0, 0)
// tools/lab/stream_mx_lab.hip: timing-only ablations of the MX main loop (profiles/stream_mx_ablation.txt).  Each takes one part out
// and leaves the rest as shipped; the scores are wrong with any of them, and none is ever defined for the library.
//   GEMM_LAB_NO_MFMA        the MFMAs (their operands are still read and converted)
//   GEMM_LAB_MX_NO_CVT      the fp8 -> bf16 conversions (the raw dwords feed the MFMA)
//   GEMM_LAB_MX_NO_AREAD    the A-fragment reads (a register stands in)
//   GEMM_LAB_MX_NO_BREAD    the B-fragment reads
//   GEMM_LAB_NO_BARRIER     the per-step s_barrier (the counted vmcnt stays)
//   GEMM_LAB_MX_BRANCHY     (not an ablation: same scores) the DMA requests of a step behind wave-uniform branches, as before the wave
//                           index was masked -- the form the table's "parent" rows were measured on
#if defined(GEMM_LAB_NO_MFMA)
#define STREAM_MX_MMA(FIRST_, a, b, c)                                                                            \
    do {                                                                                                          \
        if (FIRST_) { _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) (c)[r_] = 0; }                            \
        asm volatile("" :: "v"((a).x), "v"((a).y), "v"((a).z), "v"((a).w), "v"((b).x), "v"((b).y), "v"((b).z), "v"((b).w)); \
    } while (0)
#else
#define STREAM_MX_MMA(FIRST_, a, b, c) do { if (FIRST_) (c) = mma0<1>((a), (b)); else mma<1>((a), (b), (c)); } while (0)
#endif
#if defined(GEMM_LAB_MX_NO_CVT)
#define STREAM_MX_CVT(w0, w1) make_uint4((w0), (w0), (w1), (w1))
#else
#define STREAM_MX_CVT(w0, w1) make_uint4(fp8x2_bf16((w0), false), fp8x2_bf16((w0), true), fp8x2_bf16((w1), false), fp8x2_bf16((w1), true))
#endif
#if defined(GEMM_LAB_MX_NO_AREAD)   // (the reads in front of it lose their only use and are dropped)
#define STREAM_MX_LAB_A(arr) do { _Pragma("unroll") for (int i_ = 0; i_ < RI; ++i_) (arr)[i_] = lab_frag; } while (0)
#else
#define STREAM_MX_LAB_A(arr) do { } while (0)
#endif
#if defined(GEMM_LAB_MX_NO_BREAD)
#define STREAM_MX_LAB_B(b0, b1) do { _Pragma("unroll") for (int j_ = 0; j_ < CJ; ++j_) { (b0)[j_] = lab_frag; (b1)[j_] = lab_frag; } } while (0)
#else
#define STREAM_MX_LAB_B(b0, b1) do { } while (0)
#endif
typedef float v2f __attribute__((ext_vector_type(2)));
// One fp32 fma as ONE VALU instruction.  Measured (tools/lab/pair_probe): packed fp32 math (v_pk_fma_f32, v_pk_mul_f32,
// v_pk_add_f32) does not issue while the SIMD's other wave has MFMAs in flight -- a packed epilogue serialises with the
// partner's MFMA phase -- whereas plain v_fma_f32 runs in their shadow at ~0.85 of its stand-alone rate.  The asm keeps the
// SLP vectoriser from pairing two of these back into a packed op.
__device__ __forceinline__ float fma1(float a, float b, float c) {
    float d;
    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

__device__ __forceinline__ int swz3(int row, int slot) { return row * BK3 + ((slot ^ ((row >> 2) & 3)) << 4); }

template <int DT> __device__ __forceinline__ typename Acc<DT>::type mma0(const uint4& a, const uint4& b) {
    typename Acc<DT>::type z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0;
    mma<DT>(a, b, z);
    return z;
}

struct StreamTile { int mt, nt, g; };
__device__ __forceinline__ float4 lds_f4(const float* __restrict__ base, int off) { return *reinterpret_cast<const float4*>(base + off); }

// Fragment read through a __restrict__ stage pointer: the load carries alias-scope metadata, which keeps the compiler's
// waitcnt pass from ordering it behind the (untagged) in-flight LDS-DMA with a vmcnt(0); the hand-written counted vmcnt
// in front of each step's barrier is what orders them.
__device__ __forceinline__ uint4 lds_frag(const uint8_t* __restrict__ stage, int off) {
    return *reinterpret_cast<const uint4*>(stage + off);
}

// Two shapes of the same kernel:
//   NW = 4 waves, tile (64*RI) x 256, RI <= 2, 3-stage ring, 79 KiB of LDS -> TWO workgroups per CU (small K: the other
//          workgroup's main loop covers this one's epilogue);
//          (eight waves x 128 x 256 at two per CU -- four waves per SIMD, 128 VGPRs -- measured 8-12 % slower);
//   NW = 8 waves, tile (64*RI) x 256, RI = 3 or 4, 4-stage ring, <= 138 KiB -> one workgroup per CU (large K: the main
//          loop is bound by the L2 -> LDS DMA path, measured ~30 B/clk/CU, and the 192/256-row tile moves 23/33 % fewer
//          operand bytes per MAC; the epilogue is < 10 % of such a tile).
// Waves form a 2 x (NW/2) grid; each owns RI x CJ MFMA tiles (CJ = 16/NW), 128 accumulator registers at most.
// MX (round 3; DT = 1, the wide form): MIXED operands -- A rows bf16, B columns fp8 e4m3 (exact small integers: the weight
// candidates of a <= 4-bit search against AdaLog-quantised activations, reference linear.py:355-392 for the post-GELU layer).
// A step then covers 64 K elements: TWO 64-byte planes of A rows and ONE 64-byte K-step of B columns, 3/4 of the bytes the
// all-bf16 launch moves through the L2 -> LDS path that bounds this kernel.  The fp8 fragments are converted in registers
// (v_cvt_scalef32_pk_bf16_fp8: exact); lane -> K mapping of sub-step m:  K = 32 (m >> 1) + 16 fkg + 8 (m & 1) + 0..7.
template <int DT, int RI, int NW, int NS = (NW == 4 ? 3 : 4), bool MX = false>
__global__ __launch_bounds__(64 * NW, (NS == 3 && !MX) ? (NW == 8 ? 4 : 2) : 1) void k_gemm_stream(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)   // the buffer-resource type and builtins exist only in the device pass
    static_assert(!MX || (DT == 1 && NW == 8), "mixed operands: bf16 rows, the 8-wave form");
    constexpr int NT3 = 64 * NW;                     // threads
    constexpr int CJ = 16 / NW;                      // column MFMA tiles per wave
    constexpr int WCOLS = CJ * 32;                   // columns per wave
    constexpr int BM3 = 64 * RI;
    constexpr int APL = BM3 / 16;                    // 16-row DMA requests of one 64-byte plane of the A tile
    constexpr int AP = MX ? 2 * APL : APL;           // ... of the A tile per K-step; B has 16
    constexpr int STAGE3 = ((MX ? 2 : 1) * BM3 + BN2) * BK3;
    constexpr int PT = AP + 16;
    constexpr int MAXQ = (PT + NW - 1) / NW;         // requests per wave per K-step (the first PT % NW waves own MAXQ)
    extern __shared__ __attribute__((aligned(16))) uint8_t ring[];   // NS * STAGE3 bytes (dynamic: keeps the DMA untagged)
    __shared__ __attribute__((aligned(16))) float s_ref[4 * BM3];     // [nref <= 4][BM3]: ref - row_bias (- column bias if shared)
    __shared__ __attribute__((aligned(16))) float s_rs[BM3];          // row scale, 0 past M
    __shared__ __attribute__((aligned(16))) float s_w[BM3];           // 1 for rows < M else 0
    __shared__ float s_alpha[BN2], s_beta[BN2];                       // per column: -(sa*sb), column bias; 0 past N
    __shared__ float s_red[2][BN2];

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = w / (NW / 2), wc = w % (NW / 2);
    // Owner index of the DMA requests.  MX: masked to 0 .. NW - 1 (which it is), so that whether request w + q * NW of a step reads A or
    // B rows is a compile-time fact.  The wave-uniform branches that decided it at run time cut every K-step into a dozen basic blocks,
    // and no fragment read or conversion could be scheduled across them: each sub-step's ds_reads sat right in front of the MFMAs
    // that consume them (profiles/stream_mx_ablation.txt: 0.65 -> 0.60 ms per fc2 launch with the K-step in one block).
#if defined(GEMM_LAB_MX_BRANCHY)
    const int wq = w;
#else
    const int wq = MX ? (w & (NW - 1)) : w;
#endif
#if defined(GEMM_LAB_MX_NO_AREAD) || defined(GEMM_LAB_MX_NO_BREAD)
    uint4 lab_frag = make_uint4(lane, lane, lane, lane);
    asm volatile("" : "+v"(lab_frag.x), "+v"(lab_frag.y), "+v"(lab_frag.z), "+v"(lab_frag.w));
#endif
    const int frow = lane & 31, fkg = lane >> 5;
    const int arow = wr * (BM3 / 2) + frow, brow = wc * WCOLS + frow;

    // ---- tile list of this workgroup: the XCD it runs on owns a contiguous range of tiles (neighbours share operand
    // tiles in that XCD's L2); its workgroups take them round-robin.
    const unsigned T = (unsigned)p.MT * p.NT * p.G;
    const unsigned nwg = gridDim.x, bid = blockIdx.x, xcd = bid & 7;
    const unsigned q8 = T >> 3, r8 = T & 7;
    const unsigned t_lo = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
    const unsigned t_cnt = q8 + (xcd < r8 ? 1u : 0u);
    const unsigned nj = (nwg >> 3) + (xcd < (nwg & 7) ? 1u : 0u);
    const unsigned j0 = bid >> 3;
    auto decode = [&](unsigned local) {
        unsigned t = t_lo + local;
        StreamTile r;
        if (p.order == 2) {
            // grouped: within a group of gm m-tiles the m index runs fastest, then n; the group's A rows (<= ~2 MiB)
            // stay in the XCD's L2 while the B tiles stream through once per group
            const unsigned per_g = (unsigned)p.MT * p.NT;
            r.g = t / per_g; t -= r.g * per_g;
            const unsigned grp = t / ((unsigned)p.gm * p.NT), first = grp * p.gm;
            const unsigned gsz = min((unsigned)p.gm, (unsigned)p.MT - first);
            t -= grp * p.gm * p.NT;
            r.nt = t / gsz; r.mt = first + (t - r.nt * gsz);
        } else { r.nt = t % p.NT; t /= p.NT; r.mt = t % p.MT; r.g = t / p.MT; }
        return r;
    };
    const int nk = (int)((p.Kvb + BK3 - 1) / BK3);          // whole 64-byte steps of zero padding are skipped
    const int Kb = (int)p.Kb;
    const int KbA = MX ? (int)p.KbA : Kb;                   // (mixed: bf16 rows of 2 x the fp8 columns' bytes)

    // ---- issue cursor: runs NS - 1 K-steps ahead of the compute cursor, across tile boundaries.  Request r of a step
    // covers 16 rows x 64 bytes and lands at stage + r * 1024 (A rows first, then B rows); wave w owns r = w + q * NW.
    // Per request the lane's source is  row * Kb + 16 * (logical slot);  LDS destinations are lane-linear, so the bank
    // swizzle goes into the source slot: lane l lands in (row l>>2, physical slot l&3) = logical slot (l&3) ^ ((l>>4)&3).
    const int lrow = lane >> 2, lslot16 = ((lane & 3) ^ ((lane >> 4) & 3)) << 4;
    __amdgpu_buffer_rsrc_t ra, rb;
    int vo[MAXQ];
    unsigned i_local = j0;
    int i_k = 0;
    auto issue_tile = [&](unsigned local) {
        const StreamTile t = decode(local);
        const int m0 = t.mt * BM3, n0 = t.nt * BN2;
        ra = __builtin_amdgcn_make_buffer_rsrc((void*)(p.A + (int64_t)t.g * p.sAg + (int64_t)m0 * KbA), 0, 0x7ffffffe, 0x00020000);
        rb = __builtin_amdgcn_make_buffer_rsrc((void*)(p.B + (int64_t)t.g * p.sBg + (int64_t)n0 * Kb), 0, 0x7ffffffe, 0x00020000);
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) {
            const int r = wq + q * NW;                      // wave-uniform
            const bool isA = r < AP;
            int row = (isA ? (MX ? r % APL : r) : r - AP) * 16 + lrow;
            row = min(row, isA ? p.M - 1 - m0 : p.N - 1 - n0);   // edge rows: re-read the last valid row (masked in the epilogue)
            vo[q] = isA ? row * KbA + (MX ? (r / APL) * BK3 : 0) + lslot16 : row * Kb + lslot16;
        }
    };
    auto issue_advance = [&]() {
        if (++i_k == nk) {
            i_k = 0;
            if (i_local + nj < t_cnt) { i_local += nj; issue_tile(i_local); }   // past the last tile: harmless re-fetch
        }
    };
    auto issue_slot = [&](int q, uint8_t* st, int ko) {
        const int r = wq + q * NW;
        if (PT % NW == 0 || q + 1 < MAXQ || r < PT) {
            if (r < AP) STREAM_DMA(ra, st + r * 1024, vo[q], MX ? 2 * ko : ko);
            else STREAM_DMA(rb, st + r * 1024, vo[q], ko);
        }
    };
    issue_tile(i_local);
#pragma unroll
    for (int s0 = 0; s0 < NS - 1; ++s0) {                   // prologue: the first NS - 1 steps
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) issue_slot(q, ring + s0 * STAGE3, i_k * BK3);
        issue_advance();
    }

    const int rsh = __ffs(p.ref_div) - 1, rmask = p.ref_div - 1;   // ref_div is 64, 128 or 256 here
    const int nref = BN2 >> rsh;                            // reference columns per tile (<= 4)
    const int n_eff = p.N >> rsh;
    const bool beta_staged = p.bias && p.bi_c == 0;         // column bias independent of the candidate: fold into s_ref
    const bool beta_cols = p.bias && p.bi_c != 0;
    const bool rows = p.row_scale != nullptr;
    int st = 0;                                             // ring slot of the current step
    typename Acc<DT>::type acc[RI][CJ];
    // per-workgroup accumulation (wg_acc): thread t < 256 owns tile column t; its running fp64 sum covers this workgroup's
    // tiles of one head in their fixed order and is flushed into [workgroup][head][t] when the head changes
    double run = 0.0;
    int run_h = -1;
    if (p.wg_acc && tid < BN2)
        for (int h = 0; h < p.gmod; ++h) p.wg_acc[((int64_t)bid * p.gmod + h) * BN2 + tid] = 0.0;

    // One 64-byte K-step = 2 sub-steps of (RI + CJ) fragment reads and RI x CJ MFMAs.  Both sub-steps' fragments are read
    // up front; this wave's DMA requests for the step NS - 1 ahead are issued between the MFMA groups.
#define STREAM_STEP(FIRST, cur, nxt, ko)                                                                   \
    do {                                                                                                   \
      if constexpr (MX) {                                                                                  \
        const uint8_t* Bx_ = (cur) + 2 * BM3 * BK3;                                                        \
        uint4 q0[CJ], q1[CJ];                                                                              \
        _Pragma("unroll") for (int j = 0; j < CJ; ++j) {                                                   \
            q0[j] = lds_frag(Bx_, swz3(brow + j * 32, fkg)); q1[j] = lds_frag(Bx_, swz3(brow + j * 32, 2 + fkg)); \
        }                                                                                                  \
        STREAM_MX_LAB_B(q0, q1);                                                                           \
        _Pragma("unroll") for (int m = 0; m < 4; ++m) {                                                    \
            const uint8_t* Ap_ = (cur) + (m >> 1) * (BM3 * BK3);                                           \
            uint4 am[RI], bm[CJ];                                                                          \
            _Pragma("unroll") for (int i = 0; i < RI; ++i) am[i] = lds_frag(Ap_, swz3(arow + i * 32, 2 * fkg + (m & 1))); \
            STREAM_MX_LAB_A(am);                                                                           \
            _Pragma("unroll") for (int j = 0; j < CJ; ++j) {                                               \
                const uint4 s_ = (m >> 1) ? q1[j] : q0[j];                                                 \
                const uint32_t w0_ = (m & 1) ? s_.z : s_.x, w1_ = (m & 1) ? s_.w : s_.y;                   \
                bm[j] = STREAM_MX_CVT(w0_, w1_);                                                           \
            }                                                                                              \
            _Pragma("unroll") for (int j = 0; j < CJ; ++j) {                                               \
                _Pragma("unroll") for (int i = 0; i < RI; ++i) STREAM_MX_MMA(FIRST && m == 0, am[i], bm[j], acc[i][j]); \
                _Pragma("unroll") for (int q = m * CJ + j; q < MAXQ; q += 4 * CJ) issue_slot(q, (nxt), (ko)); \
            }                                                                                              \
        }                                                                                                  \
      } else {                                                                                             \
        const uint8_t* Bs_ = (cur) + BM3 * BK3;                                                            \
        uint4 a0[RI], b0[CJ], a1[RI], b1[CJ];                                                              \
        _Pragma("unroll") for (int i = 0; i < RI; ++i) a0[i] = lds_frag((cur), swz3(arow + i * 32, fkg));  \
        _Pragma("unroll") for (int j = 0; j < CJ; ++j) b0[j] = lds_frag(Bs_, swz3(brow + j * 32, fkg));    \
        _Pragma("unroll") for (int i = 0; i < RI; ++i) a1[i] = lds_frag((cur), swz3(arow + i * 32, 2 + fkg)); \
        _Pragma("unroll") for (int j = 0; j < CJ; ++j) b1[j] = lds_frag(Bs_, swz3(brow + j * 32, 2 + fkg)); \
        if constexpr (DT == 3) {                                                                           \
            _Pragma("unroll") for (int j = 0; j < CJ; ++j) {                                               \
                _Pragma("unroll") for (int i = 0; i < RI; ++i) {                                           \
                    v16f z_;                                                                               \
                    _Pragma("unroll") for (int r = 0; r < 16; ++r) z_[r] = 0.0f;                           \
                    acc[i][j] = mma_fp8x64(a0[i], a1[i], b0[j], b1[j], FIRST ? z_ : acc[i][j]);            \
                }                                                                                          \
                _Pragma("unroll") for (int q = j; q < MAXQ; q += CJ) issue_slot(q, (nxt), (ko));           \
            }                                                                                              \
        } else {                                                                                           \
            _Pragma("unroll") for (int j = 0; j < CJ; ++j) {                                               \
                _Pragma("unroll") for (int i = 0; i < RI; ++i) {                                           \
                    if (FIRST) acc[i][j] = mma0<DT == 3 ? 1 : DT>(a0[i], b0[j]);                           \
                    else mma<DT == 3 ? 1 : DT>(a0[i], b0[j], acc[i][j]);                                   \
                }                                                                                          \
                _Pragma("unroll") for (int q = j; q < MAXQ; q += 2 * CJ) issue_slot(q, (nxt), (ko));       \
            }                                                                                              \
            _Pragma("unroll") for (int j = 0; j < CJ; ++j) {                                               \
                _Pragma("unroll") for (int i = 0; i < RI; ++i) mma<DT == 3 ? 1 : DT>(a1[i], b1[j], acc[i][j]); \
                _Pragma("unroll") for (int q = CJ + j; q < MAXQ; q += 2 * CJ) issue_slot(q, (nxt), (ko));  \
            }                                                                                              \
        }                                                                                                  \
      }                                                                                                    \
    } while (0)

    for (unsigned local = j0; local < t_cnt; local += nj) {
        const StreamTile tl = decode(local);
        const int g = tl.g, gh = g % p.gmod, m0 = tl.mt * BM3, n0 = tl.nt * BN2;
        const int ni0 = n0 >> rsh;
        const bool edge = (m0 + BM3 > p.M) || (n0 + BN2 > p.N);
        [[maybe_unused]] const unsigned lid = t_lo + local;
        TL_STAMP(0);
        for (int kt = 0; kt < nk; ++kt) {
            // stage `st` has landed once only the newest NS - 2 steps' requests of this wave are still outstanding
            if (PT % NW != 0 && w >= PT % NW) {
                if ((NS - 2) * (MAXQ - 1) == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
                else if ((NS - 2) * (MAXQ - 1) == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else if ((NS - 2) * (MAXQ - 1) == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            } else {
                if ((NS - 2) * MAXQ == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
                else if ((NS - 2) * MAXQ == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                else if ((NS - 2) * MAXQ == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
#if !defined(GEMM_LAB_NO_BARRIER)
            __builtin_amdgcn_s_barrier();
#endif
            asm volatile("" ::: "memory");
            const int stn = st == 0 ? NS - 1 : st - 1;       // (st + NS - 1) % NS: the slot read in the previous step
            const int ko = i_k * BK3;
            if (kt == 0) {
                TL_STAMP(1);
                // ---- epilogue operands of this tile: plain loads now (clamped addresses, no dependent arithmetic, so
                // nothing waits before the MFMAs), masks + arithmetic + LDS staging writes after the step
                const float* refg = p.ref + (int64_t)g * p.sRg;
                const int rcs = (int)p.ref_cs;
                constexpr int EU = (4 * BM3 + NT3 - 1) / NT3;
                float e_ref[EU], e_rb[EU], e_cb[EU];
#pragma unroll
                for (int u = 0; u < EU; ++u) {
                    const int e = min(tid + u * NT3, 4 * BM3 - 1);
                    const int nl = e / BM3, rl = e - nl * BM3;
                    const int rowc = min(m0 + rl, p.M - 1), nic = min(ni0 + nl, n_eff - 1);
#if defined(GEMM_LAB_ELOAD_HOT)   // lab: always-cached address, to tell load latency from instruction overhead
                    e_ref[u] = refg[(rowc + nic * rcs) & 1023];
#else
                    e_ref[u] = refg[rowc + nic * rcs];
#endif
                    e_rb[u] = p.row_bias ? p.row_bias[rowc] : 0.0f;
                    e_cb[u] = beta_staged ? p.bias[gh * p.bi_g + nic * p.bi_n] : 0.0f;
                }
                const int rrow = min(m0 + min(tid, BM3 - 1), p.M - 1);
                const float e_rs = rows ? p.row_scale[rrow] : 1.0f;
                const int colc = min(n0 + min(tid, BN2 - 1), p.N - 1);
                const int cci = colc & rmask, cni = colc >> rsh;
                const float e_sa = p.sa[cci * p.sa_c + gh * p.sa_g];
                const float e_sb = p.sb[cci * p.sb_c + gh * p.sb_g + cni * p.sb_n];
                const float e_be = beta_cols ? p.bias[cci * p.bi_c + gh * p.bi_g + cni * p.bi_n] : 0.0f;
                STREAM_STEP(true, ring + st * STAGE3, ring + stn * STAGE3, ko);
#pragma unroll
                for (int u = 0; u < EU; ++u) {
                    const int e = tid + u * NT3;
                    const int nl = e / BM3, rl = e - nl * BM3;
                    const bool ok = (m0 + rl < p.M) && (ni0 + nl < n_eff);
                    if (e < nref * BM3) s_ref[e] = ok ? (e_ref[u] - e_rb[u]) - e_cb[u] : 0.0f;
                }
                if (tid < BM3) {
                    const bool ok = m0 + tid < p.M;
                    s_rs[tid] = ok ? e_rs : 0.0f;
                    s_w[tid] = ok ? 1.0f : 0.0f;
                }
                if (tid < BN2) {
                    const bool ok = n0 + tid < p.N;
                    s_alpha[tid] = ok ? -(e_sa * p.sa_mul * e_sb) : 0.0f;
                    s_beta[tid] = ok ? e_be : 0.0f;
                }
                TL_STAMP(2);
            } else {
                STREAM_STEP(false, ring + st * STAGE3, ring + stn * STAGE3, ko);
            }
            issue_advance();
            st = st == NS - 1 ? 0 : st + 1;
        }
        TL_STAMP(3);

        // ---- epilogue.  The staging written after the first step must be visible: with nk >= 2 a later step's barrier
        // already separates them.
        if (nk == 1) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        v2f cs2[CJ];
        float nal[CJ], bet[CJ], cm[CJ];
        const float* rj[CJ];
#pragma unroll
        for (int j = 0; j < CJ; ++j) {
            const int cl = wc * WCOLS + j * 32 + frow;
            nal[j] = s_alpha[cl]; bet[j] = s_beta[cl];
            cm[j] = (n0 + cl < p.N) ? 1.0f : 0.0f;
            rj[j] = s_ref + (cl >> rsh) * BM3;
            cs2[j] = (v2f){0.0f, 0.0f};
        }
        const bool full = edge || beta_cols;                // generic body: row weights and column bias applied
#define STREAM_EPILOGUE(ROWS_, FULL_)                                                                          \
        _Pragma("unroll") for (int i = 0; i < RI; ++i) {                                                       \
            _Pragma("unroll") for (int q4 = 0; q4 < 4; ++q4) {                                                 \
                const int rl = wr * (BM3 / 2) + i * 32 + 4 * fkg + 8 * q4;                                     \
                float4 s4 = make_float4(1.f, 1.f, 1.f, 1.f), w4 = s4;                                          \
                if (ROWS_) s4 = *reinterpret_cast<const float4*>(s_rs + rl);                                   \
                if (FULL_) w4 = *reinterpret_cast<const float4*>(s_w + rl);                                    \
                const v2f sA = {s4.x, s4.y}, sB = {s4.z, s4.w}, wA = {w4.x, w4.y}, wB = {w4.z, w4.w};          \
                _Pragma("unroll") for (int j = 0; j < CJ; ++j) {                                               \
                    const float4 r4 = *reinterpret_cast<const float4*>(rj[j] + rl);                            \
                    v2f rA = {r4.x, r4.y}, rB = {r4.z, r4.w};                                                  \
                    v2f tA = {(float)acc[i][j][q4 * 4 + 0], (float)acc[i][j][q4 * 4 + 1]};                     \
                    v2f tB = {(float)acc[i][j][q4 * 4 + 2], (float)acc[i][j][q4 * 4 + 3]};                     \
                    const v2f na = {nal[j], nal[j]};                                                           \
                    if (ROWS_) { tA *= sA; tB *= sB; }                                                         \
                    if (FULL_) { const v2f b2 = {bet[j], bet[j]}; rA -= b2; rB -= b2; }                        \
                    v2f dA = tA * na + rA, dB = tB * na + rB;                                                  \
                    if (FULL_) { dA *= wA; dB *= wB; }                                                         \
                    cs2[j] += dA * dA; cs2[j] += dB * dB;                                                      \
                }                                                                                              \
            }                                                                                                  \
        }
        // ref_div >= 128: the wave's CJ * 32 columns share ONE reference column, so a row group needs one float4 of the
        // staged reference (not CJ); the next group's LDS values are fetched before the current group's arithmetic (the
        // epilogue was LDS-latency-bound: ~4.2 k cycles for ~300 VALU, with or without the int->float conversions).
#define STREAM_EPILOGUE_SAME(ROWS_, FULL_)                                                                     \
        {                                                                                                      \
            constexpr int NG_ = RI * 4;                                                                        \
            const float* rbase_ = rj[0] + wr * (BM3 / 2) + 4 * fkg;                                            \
            const float* sbase_ = s_rs + wr * (BM3 / 2) + 4 * fkg;                                             \
            const float* wbase_ = s_w + wr * (BM3 / 2) + 4 * fkg;                                              \
            float4 r_n = *reinterpret_cast<const float4*>(rbase_), s_n = make_float4(1.f, 1.f, 1.f, 1.f), w_n = s_n; \
            if (ROWS_) s_n = *reinterpret_cast<const float4*>(sbase_);                                         \
            if (FULL_) w_n = *reinterpret_cast<const float4*>(wbase_);                                         \
            _Pragma("unroll") for (int gi = 0; gi < NG_; ++gi) {                                               \
                const int i = gi >> 2, q4 = gi & 3;                                                            \
                const float4 r4 = r_n, s4 = s_n, w4 = w_n;                                                     \
                if (gi + 1 < NG_) {                                                                            \
                    const int o_ = ((gi + 1) >> 2) * 32 + 8 * ((gi + 1) & 3);                                  \
                    r_n = *reinterpret_cast<const float4*>(rbase_ + o_);                                       \
                    if (ROWS_) s_n = *reinterpret_cast<const float4*>(sbase_ + o_);                            \
                    if (FULL_) w_n = *reinterpret_cast<const float4*>(wbase_ + o_);                            \
                }                                                                                              \
                const v2f sA = {s4.x, s4.y}, sB = {s4.z, s4.w}, wA = {w4.x, w4.y}, wB = {w4.z, w4.w};          \
                _Pragma("unroll") for (int j = 0; j < CJ; ++j) {                                               \
                    v2f rA = {r4.x, r4.y}, rB = {r4.z, r4.w};                                                  \
                    v2f tA = {(float)acc[i][j][q4 * 4 + 0], (float)acc[i][j][q4 * 4 + 1]};                     \
                    v2f tB = {(float)acc[i][j][q4 * 4 + 2], (float)acc[i][j][q4 * 4 + 3]};                     \
                    const v2f na = {nal[j], nal[j]};                                                           \
                    if (ROWS_) { tA *= sA; tB *= sB; }                                                         \
                    if (FULL_) { const v2f b2 = {bet[j], bet[j]}; rA -= b2; rB -= b2; }                        \
                    v2f dA = tA * na + rA, dB = tB * na + rB;                                                  \
                    if (FULL_) { dA *= wA; dB *= wB; }                                                         \
                    cs2[j] += dA * dA; cs2[j] += dB * dB;                                                      \
                }                                                                                              \
            }                                                                                                  \
        }
        if (p.ref_div >= WCOLS) {
            if (full) STREAM_EPILOGUE_SAME(true, true)
            else if (rows) STREAM_EPILOGUE_SAME(true, false)
            else STREAM_EPILOGUE_SAME(false, false)
        } else {
            if (full) { STREAM_EPILOGUE(true, true) }
            else if (rows) { STREAM_EPILOGUE(true, false) }
            else { STREAM_EPILOGUE(false, false) }
        }
#undef STREAM_EPILOGUE_SAME
#undef STREAM_EPILOGUE
#pragma unroll
        for (int j = 0; j < CJ; ++j) {
            float cs = (cs2[j].x + cs2[j].y) * cm[j];
            cs += __shfl_xor(cs, 32);
            if (fkg == 0) s_red[wr][wc * WCOLS + j * 32 + frow] = cs;
        }
        TL_STAMP(4);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // not __syncthreads(): its fence would drain the DMA
        TL_STAMP(5);
        if (tid < BN2) {
            const int col = n0 + tid;
            const float v = s_red[0][tid] + s_red[1][tid];         // 0 for columns past N (masked above)
            if (p.wg_acc) {
                if (gh != run_h) {
                    if (run_h >= 0) p.wg_acc[((int64_t)bid * p.gmod + run_h) * BN2 + tid] += run;
                    run = 0.0; run_h = gh;
                }
                run += (double)v;
            } else if (col < p.N) {
                p.partial[((((int64_t)g) * p.MT + tl.mt) * p.Npad + (col >> rsh)) * p.ref_div + (col & rmask)] = v;
            }
        }
        TL_STAMP(6);
        TL_STAMP(7);
    }
    if (p.wg_acc && tid < BN2 && run_h >= 0) p.wg_acc[((int64_t)bid * p.gmod + run_h) * BN2 + tid] += run;
#undef STREAM_STEP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // drain the run-ahead steps before the LDS is released
#endif
}

