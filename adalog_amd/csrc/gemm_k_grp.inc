// Part of gemm_score.hip (one translation unit, included inside its anonymous namespace): group kernels of the attention searches (q.k^T: one K-step; softmax.v: seven).
// ------------------------------------------------------------------------------------------------ group kernel
// Fifth form, for the attention q.k^T searches: many small groups (image x head), one 64-byte K-step, 129..224 rows.
// k_gemm_stream spends such a tile on its epilogue and its per-tile set-up (2 MFMAs per 32 x 32 outputs against ~32
// VALU), at 0.4 PFLOP/s.  Here a workgroup is 7 consumer waves + 1 loader wave:
//   * consumer w keeps the fragments of row block w of the current group in REGISTERS (8 VGPRs) for a whole item
//     (= group x chunk of candidate columns) together with the 16 reference values per reference column it needs;
//   * the loader wave alone issues the LDS-DMA of the candidate columns (stages of 256 columns = 16 KiB, 3-stage ring)
//     and is the only wave that counts vmcnt; one workgroup barrier per stage hands a stage over;
//   * per 32 x 32 block a consumer does 2 ds_read_b128, 2 MFMAs and the 32-VALU epilogue; column sums stay in registers
//     for the item, then go through LDS into per-workgroup fp64 sums per head (fixed order: no atomics).
// Output: the wg_acc layout of k_gemm_stream ([workgroup][head][256] fp64), same number of workgroups.
typedef unsigned v4u __attribute__((ext_vector_type(4)));

template <int NJ, int DT>
__global__ __launch_bounds__(512, NJ == 8 ? 2 : 4) void k_gemm_grp(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int NSG = 3, SB = 8, SBYTES = SB * 32 * BK3;     // ring stages, blocks per stage, bytes per stage
    constexpr int P = NJ * 32;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t* ring = lds;                                                        // [NSG][256 columns][64 bytes]
    float* red = reinterpret_cast<float*>(lds + NSG * SBYTES);                  // [7 waves][256]
    double* accl = reinterpret_cast<double*>(lds + NSG * SBYTES + 7 * 256 * 4); // [gmod][256]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fkg = lane >> 5;
    const int Kb = (int)p.Kb;
    const int NB = p.N >> 5;                                  // 32-column blocks per group
    const int CB = p.slab_R, NCH = p.slab_U;                  // blocks per chunk, chunks per group
    const int items = p.G * NCH;
    const int n_eff = p.N / P;
    for (int i = tid; i < p.gmod * 256; i += 512) accl[i] = 0.0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // ---------------- issue side (every wave): the stages of this workgroup's items, two ahead of the compute side.
    // A stage is 16 requests of 16 columns x 64 bytes.  Issuing one costs a wave ~100 cycles, so a single loader wave
    // (1 600 cycles per stage against ~900 of consumer work) was the bottleneck: the loader keeps requests 7..15 and
    // consumer w issues request w (an even split, two per wave, measured 5 % slower).
    const int lrow = lane >> 2, lslot16 = ((lane & 3) ^ ((lane >> 4) & 3)) << 4;
    int li = blockIdx.x, lst = 0, slot = 0;                   // item / stage cursor of the issue side
    int ahead = 0;                                             // stages issued and not yet handed over
    auto stages_of = [&](int item) { const int c = item % NCH; return (min(CB, NB - c * CB) + SB - 1) / SB; };
    auto issue = [&]() {
        const int g = li / NCH, c = li - g * NCH;
        const int col0 = (c * CB + lst * SB) * 32;
        const int64_t left = (int64_t)(p.N - col0) * Kb;
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(p.B + (int64_t)g * p.sBg + (int64_t)col0 * Kb), 0,
                                                                            (int)(left < 0 ? 0 : min(left, (int64_t)0x7ffffffe)), 0x00020000);
        uint8_t* st = ring + slot * SBYTES;
        if (w == 7) {
#pragma unroll
            for (int q = 7; q < 16; ++q) STREAM_DMA(rb, st + q * 1024, (q * 16 + lrow) * Kb + lslot16, 0);
        } else STREAM_DMA(rb, st + w * 1024, (w * 16 + lrow) * Kb + lslot16, 0);
        slot = slot == NSG - 1 ? 0 : slot + 1;
        if (++lst == stages_of(li)) { lst = 0; li += gridDim.x; }
        ++ahead;
    };
    if (li < items) issue();
    if (li < items) issue();

    if (w == 7) {
        // ---------------- loader wave: nothing but its share of the requests
        for (int item = blockIdx.x; item < items; item += gridDim.x) {
            const int ns = stages_of(item);
            for (int t = 0; t < ns; ++t) {
                if (ahead >= 2) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");    // the following stage's nine may be in flight
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                asm volatile("s_barrier" ::: "memory");
                --ahead;
                if (li < items) issue();
            }
            asm volatile("s_barrier" ::: "memory");                        // item end: column sums are in `red`
        }
    } else {
        // ---------------- consumers: row block w
        const int row0 = w * 32;
        const bool rowblock_live = row0 < p.M;                 // (always true for the launches this kernel takes)
        int st = 0;                                            // ring slot of the next stage (runs on across items)
        for (int item = blockIdx.x; item < items; item += gridDim.x) {
            const int g = item / NCH, c = item - g * NCH, gh = g % p.gmod;
            const int blk0 = c * CB, nblk = min(CB, NB - blk0), ns = (nblk + SB - 1) / SB;
            // fragments of this row block (rows past M are zero), column factors of the group's head
            uint4 a0, a1;
            {
                const bool ok = row0 + frow < p.M;
                const uint8_t* ar = p.A + (int64_t)g * p.sAg + (int64_t)min(row0 + frow, p.M - 1) * Kb;
                a0 = *reinterpret_cast<const uint4*>(ar + fkg * 16);
                a1 = *reinterpret_cast<const uint4*>(ar + 32 + fkg * 16);
                if (!ok) { a0 = make_uint4(0, 0, 0, 0); a1 = a0; }
            }
            float nal[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int ci = j * 32 + frow;
                nal[j] = -(p.sa[ci * p.sa_c + gh * p.sa_g] * p.sa_mul * p.sb[ci * p.sb_c + gh * p.sb_g]);
            }
            // reference slice of one reference column: rows row0 + 8*q + 4*fkg + {0..3}, zero past M.  One 16-byte load
            // per q from a uniform column base + a per-lane row offset clamped to M - 4; the ragged (last) row block then
            // shifts the elements it still owns into place.
            // (buffer loads: uniform column offset in an SGPR + four loop-invariant lane offsets -- with flat pointers the
            // compiler kept one 64-bit address per call site alive and spilled them)
            const uint32_t ref_bytes = (uint32_t)(((int64_t)(n_eff - 1) * p.ref_cs + p.M) * 4);   // past it a load returns 0
            const __amdgpu_buffer_rsrc_t rrg = __builtin_amdgcn_make_buffer_rsrc((void*)(p.ref + (int64_t)g * p.sRg), 0, (int)ref_bytes, 0x00020000);
            const bool full_rows = row0 + 32 <= p.M;          // wave-uniform
            int roff[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) roff[q] = min(row0 + 8 * q + 4 * fkg, p.M - 4) * 4;
            v2f cs2[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) cs2[j] = (v2f){0.0f, 0.0f};
            // The stage loop exists twice (whole / ragged row block, chosen per wave) so that its body has no branch: with
            // one, the compiler's waitcnt pass drains the reference prefetch it has just issued.
            auto run = [&](auto full_tag) {
                constexpr bool FULL = decltype(full_tag)::value;
                auto load_ref = [&](int n, float4 (&r)[4]) {
                    const int coff = n < n_eff ? n * (int)p.ref_cs * 4 : 0x7ffffff0;   // (uniform) past the last column: zeros
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const v4u uu = __builtin_amdgcn_raw_buffer_load_b128(rrg, roff[q], coff, 0);
                        r[q] = make_float4(__uint_as_float(uu.x), __uint_as_float(uu.y), __uint_as_float(uu.z), __uint_as_float(uu.w));
                    }
                };
                // ragged row block: the loaded group of four starts at min(row, M - 4); move the elements this lane owns
                // into place and zero the rows past M.  Done when a set becomes the current one, NOT at the load: there
                // it would wait for the load it has just issued (and the whole workgroup waits for this wave at the barrier).
                auto fix_ref = [&](float4 (&r)[4]) {
                    if (FULL) return;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int rr = row0 + 8 * q + 4 * fkg;
                        const float4 u = r[q];
                        const int sh = rr * 4 - roff[q];       // 0 unless the group of four crosses M (then 4, 8 or 12 bytes)
                        const float e0 = sh == 0 ? u.x : sh == 4 ? u.y : sh == 8 ? u.z : u.w;
                        const float e1 = sh == 0 ? u.y : sh == 4 ? u.z : u.w;
                        const float e2 = sh == 0 ? u.z : u.w;
                        r[q] = make_float4(rr < p.M ? e0 : 0.f, rr + 1 < p.M ? e1 : 0.f, rr + 2 < p.M ? e2 : 0.f, rr + 3 < p.M ? u.w : 0.f);
                    }
                };
                int n = blk0 / NJ;                             // chunks start on a reference column (CB % 8 == 0, NJ | 8)
                // two register sets take turns (a stage holds an even number of reference columns when NJ <= 4, so which
                // set a block reads is known at compile time; with NJ = 8 the sets are swapped by copying)
                float4 rr2[2][4];
                load_ref(n, rr2[0]);
                load_ref(n + 1, rr2[1]);
                fix_ref(rr2[0]);
                for (int t = 0; t < ns; ++t) {
                    // this wave's request of the stage has landed once only what was issued after it can be outstanding:
                    // the following stage's request and the R reference loads of the previous stage (the first stage of
                    // an item comes after the item's set-up loads: drain)
                    constexpr int R = (SB / NJ) * 4;
                    if (t == 0 || ahead < 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    else if (R == 4) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
                    else if (R == 8) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(17)" ::: "memory");
                    asm volatile("s_barrier" ::: "memory");
                    --ahead;
                    if (li < items) issue();
                    const uint8_t* cur = ring + st * SBYTES;
                    uint4 b0n = lds_frag(cur, swz3(frow, fkg)), b1n = lds_frag(cur, swz3(frow, 2 + fkg));
#pragma unroll
                    for (int b = 0; b < SB; ++b) {
                        const int j = b % NJ;
                        const int set = NJ == 8 ? 0 : (b / NJ) & 1;
                        const uint4 b0 = b0n, b1 = b1n;
                        if (b + 1 < SB) { b0n = lds_frag(cur, swz3((b + 1) * 32 + frow, fkg)); b1n = lds_frag(cur, swz3((b + 1) * 32 + frow, 2 + fkg)); }
                        typename Acc<DT == 3 ? 1 : 0>::type acc;      // fp8 operands accumulate in fp32: no conversion below
                        if constexpr (DT == 3) {
                            v16f z_;
#pragma unroll
                            for (int e = 0; e < 16; ++e) z_[e] = 0.0f;
                            acc = mma_fp8x64(a0, a1, b0, b1, z_);
                        } else {
                            acc = mma0<0>(a0, b0);
                            mma<0>(a1, b1, acc);
                        }
                        const v2f na = {nal[j], nal[j]};
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const v2f tA = {(float)acc[q * 4 + 0], (float)acc[q * 4 + 1]}, tB = {(float)acc[q * 4 + 2], (float)acc[q * 4 + 3]};
                            const v2f rA = {rr2[set][q].x, rr2[set][q].y}, rB = {rr2[set][q].z, rr2[set][q].w};
                            const v2f dA = tA * na + rA, dB = tB * na + rB;
                            cs2[j] += dA * dA; cs2[j] += dB * dB;
                        }
                        if (j == NJ - 1) {                     // next block starts the next reference column
                            ++n;
                            if (NJ == 8) {
#pragma unroll
                                for (int q = 0; q < 4; ++q) rr2[0][q] = rr2[1][q];
                                fix_ref(rr2[0]);
                                load_ref(n + 1, rr2[1]);
                            } else {
                                fix_ref(rr2[set ^ 1]);         // the other set holds column n: it becomes the current one
                                load_ref(n + 1, rr2[set]);     // this set is free now
                            }
                        }
                    }
                    st = st == NSG - 1 ? 0 : st + 1;
                }
            };
            if (!rowblock_live) {                              // (never for the launches this kernel takes)
                for (int t = 0; t < ns; ++t) {
                    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
                    --ahead;
                    if (li < items) issue();
                    st = st == NSG - 1 ? 0 : st + 1;
                }
            } else if (full_rows) run(std::true_type{});
            else run(std::false_type{});
            // item end: pair up the lanes, park the sums, one thread per candidate adds them in a fixed wave order
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                float cs = cs2[j].x + cs2[j].y;
                cs += __shfl_xor(cs, 32);
                if (fkg == 0) red[w * 256 + j * 32 + frow] = cs;
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (tid < P) {
                double v = 0.0;
                const int nw = min(7, (p.M + 31) / 32);
                for (int ww = 0; ww < nw; ++ww) v += (double)red[ww * 256 + tid];
                accl[gh * 256 + tid] += v;
            }
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int i = tid; i < p.gmod * 256; i += 512) p.wg_acc[(int64_t)blockIdx.x * p.gmod * 256 + i] = accl[i];
#endif
}

// The same organisation for groups with several K-steps (the softmax.v weight search: bf16, K = 197 keys = 7 steps, 197
// attention rows per group, 64 x P candidate columns): a consumer keeps the NK x 2 fragments of its row block in
// registers for an item, a stage is 2 column blocks x all of K (NK x 4 requests of 16 columns x 64 bytes; consumer w
// issues two of them, the loader the rest), and a block is 2 NK MFMAs against the same 16-value epilogue.
template <int NJ, int NK>
__global__ __launch_bounds__(512, 2) void k_gemm_grpk(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int NSG = 3, SB = 2, SBYTES = NK * SB * 32 * BK3;   // ring stages, blocks per stage, bytes per stage
    constexpr int RQ = NK * SB * 2, CQ = 2;                    // requests per stage, requests per consumer
    constexpr int STG = NJ / SB > 0 ? NJ / SB : 1;             // stages per reference column
    constexpr int P = NJ * 32;
    static_assert(RQ > 7 * CQ, "the loader needs a share");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t* ring = lds;                                                        // [NSG][NK][64 columns][64 bytes]
    float* red = reinterpret_cast<float*>(lds + NSG * SBYTES);                  // [7 waves][P]
    double* accl = reinterpret_cast<double*>(lds + NSG * SBYTES + 7 * P * 4);   // [gmod][256]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fkg = lane >> 5;
    const int Kb = (int)p.Kb;
    const int NB = p.N >> 5;
    const int CB = p.slab_R, NCH = p.slab_U;
    const int items = p.G * NCH;
    const int n_eff = p.N / P;
    for (int i = tid; i < p.gmod * 256; i += 512) accl[i] = 0.0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    const int lrow = lane >> 2, lslot16 = ((lane & 3) ^ ((lane >> 4) & 3)) << 4;
    int li = blockIdx.x, lst = 0, slot = 0, ahead = 0;
    auto stages_of = [&](int item) { const int c = item % NCH; return (min(CB, NB - c * CB) + SB - 1) / SB; };
    auto issue = [&]() {
        const int g = li / NCH, c = li - g * NCH;
        const int col0 = (c * CB + lst * SB) * 32;
        const int64_t left = (int64_t)(p.N - col0) * Kb;
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(p.B + (int64_t)g * p.sBg + (int64_t)col0 * Kb), 0,
                                                                            (int)(left < 0 ? 0 : min(left, (int64_t)0x7ffffffe)), 0x00020000);
        uint8_t* st = ring + slot * SBYTES;
        // request r: K-step r / 4, columns 16 * (r % 4) .. + 15
        if (w == 7) {
#pragma unroll
            for (int r = 7 * CQ; r < RQ; ++r) STREAM_DMA(rb, st + r * 1024, ((r & 3) * 16 + lrow) * Kb + lslot16, (r >> 2) * BK3);
        } else {
#pragma unroll
            for (int i = 0; i < CQ; ++i) {
                const int r = w * CQ + i;
                STREAM_DMA(rb, st + r * 1024, ((r & 3) * 16 + lrow) * Kb + lslot16, (r >> 2) * BK3);
            }
        }
        slot = slot == NSG - 1 ? 0 : slot + 1;
        if (++lst == stages_of(li)) { lst = 0; li += gridDim.x; }
        ++ahead;
    };
    if (li < items) issue();
    if (li < items) issue();

    if (w == 7) {
        for (int item = blockIdx.x; item < items; item += gridDim.x) {
            const int ns = stages_of(item);
            for (int t = 0; t < ns; ++t) {
                if (ahead >= 2) {
                    if (RQ - 7 * CQ == 14) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
                    else if (RQ - 7 * CQ == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                asm volatile("s_barrier" ::: "memory");
                --ahead;
                if (li < items) issue();
            }
            asm volatile("s_barrier" ::: "memory");
        }
    } else {
        const int row0 = w * 32;
        const bool rowblock_live = row0 < p.M;
        int st = 0;
        for (int item = blockIdx.x; item < items; item += gridDim.x) {
            const int g = item / NCH, c = item - g * NCH, gh = g % p.gmod;
            const int blk0 = c * CB, nblk = min(CB, NB - blk0), ns = (nblk + SB - 1) / SB;
            uint4 af[NK][2];
            {
                const bool ok = row0 + frow < p.M;
                const uint8_t* ar = p.A + (int64_t)g * p.sAg + (int64_t)min(row0 + frow, p.M - 1) * Kb;
#pragma unroll
                for (int kt = 0; kt < NK; ++kt) {
                    af[kt][0] = *reinterpret_cast<const uint4*>(ar + kt * BK3 + fkg * 16);
                    af[kt][1] = *reinterpret_cast<const uint4*>(ar + kt * BK3 + 32 + fkg * 16);
                    if (!ok) { af[kt][0] = make_uint4(0, 0, 0, 0); af[kt][1] = af[kt][0]; }
                }
            }
            float nal[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int ci = j * 32 + frow;
                nal[j] = -(p.sa[ci * p.sa_c + gh * p.sa_g] * p.sa_mul * p.sb[ci * p.sb_c + gh * p.sb_g]);
            }
            const uint32_t ref_bytes = (uint32_t)(((int64_t)(n_eff - 1) * p.ref_cs + p.M) * 4);
            const __amdgpu_buffer_rsrc_t rrg = __builtin_amdgcn_make_buffer_rsrc((void*)(p.ref + (int64_t)g * p.sRg), 0, (int)ref_bytes, 0x00020000);
            const bool full_rows = row0 + 32 <= p.M;
            int roff[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) roff[q] = min(row0 + 8 * q + 4 * fkg, p.M - 4) * 4;
            v2f cs2[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) cs2[j] = (v2f){0.0f, 0.0f};
            auto run = [&](auto full_tag) {
                constexpr bool FULL = decltype(full_tag)::value;
                auto load_ref = [&](int n, float4 (&r)[4]) {
                    const int coff = n < n_eff ? n * (int)p.ref_cs * 4 : 0x7ffffff0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const v4u uu = __builtin_amdgcn_raw_buffer_load_b128(rrg, roff[q], coff, 0);
                        r[q] = make_float4(__uint_as_float(uu.x), __uint_as_float(uu.y), __uint_as_float(uu.z), __uint_as_float(uu.w));
                    }
                };
                auto fix_ref = [&](float4 (&r)[4]) {
                    if (FULL) return;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int rr = row0 + 8 * q + 4 * fkg;
                        const float4 u = r[q];
                        const int sh = rr * 4 - roff[q];
                        const float e0 = sh == 0 ? u.x : sh == 4 ? u.y : sh == 8 ? u.z : u.w;
                        const float e1 = sh == 0 ? u.y : sh == 4 ? u.z : u.w;
                        const float e2 = sh == 0 ? u.z : u.w;
                        r[q] = make_float4(rr < p.M ? e0 : 0.f, rr + 1 < p.M ? e1 : 0.f, rr + 2 < p.M ? e2 : 0.f, rr + 3 < p.M ? u.w : 0.f);
                    }
                };
                int n = blk0 / NJ;
                float4 rc[4], rn[4];                           // current / next reference column
                load_ref(n, rc);
                load_ref(n + 1, rn);
                fix_ref(rc);
                for (int tg = 0; tg < ns; tg += STG) {
#pragma unroll
                    for (int s = 0; s < STG; ++s) {
                        // behind this wave's CQ requests of the stage: the next stage's CQ and the reference loads of
                        // the two stages in between (at least 8 / 4 / 0 of them for NJ = 2 / 4 / 8)
                        if ((tg == 0 && s == 0) || ahead < 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        else if (NJ == 2) { if (CQ == 2) asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); }
                        else if (NJ == 4) { if (CQ == 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); }
                        else { if (CQ == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); }
                        asm volatile("s_barrier" ::: "memory");
                        --ahead;
                        if (li < items) issue();
                        const uint8_t* cur = ring + st * SBYTES;
#pragma unroll
                        for (int b = 0; b < SB; ++b) {
                            const int j = (s * SB + b) % NJ;
                            v16f acc;
#pragma unroll
                            for (int kt = 0; kt < NK; ++kt) {
                                const uint8_t* ks = cur + kt * (SB * 32 * BK3);
                                const uint4 b0 = lds_frag(ks, swz3(b * 32 + frow, fkg)), b1 = lds_frag(ks, swz3(b * 32 + frow, 2 + fkg));
                                if (kt == 0) acc = mma0<1>(af[0][0], b0); else mma<1>(af[kt][0], b0, acc);
                                mma<1>(af[kt][1], b1, acc);
                            }
                            const v2f na = {nal[j], nal[j]};
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const v2f tA = {acc[q * 4 + 0], acc[q * 4 + 1]}, tB = {acc[q * 4 + 2], acc[q * 4 + 3]};
                                const v2f rA = {rc[q].x, rc[q].y}, rB = {rc[q].z, rc[q].w};
                                const v2f dA = tA * na + rA, dB = tB * na + rB;
                                cs2[j] += dA * dA; cs2[j] += dB * dB;
                            }
                            if (j == NJ - 1) {                 // next block starts the next reference column
                                ++n;
#pragma unroll
                                for (int q = 0; q < 4; ++q) rc[q] = rn[q];
                                fix_ref(rc);
                                load_ref(n + 1, rn);
                            }
                        }
                        st = st == NSG - 1 ? 0 : st + 1;
                    }
                }
            };
            if (!rowblock_live) {
                for (int t = 0; t < ns; ++t) {
                    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
                    --ahead;
                    if (li < items) issue();
                    st = st == NSG - 1 ? 0 : st + 1;
                }
            } else if (full_rows) run(std::true_type{});
            else run(std::false_type{});
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                float cs = cs2[j].x + cs2[j].y;
                cs += __shfl_xor(cs, 32);
                if (fkg == 0) red[w * P + j * 32 + frow] = cs;
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (tid < P) {
                double v = 0.0;
                const int nw = min(7, (p.M + 31) / 32);
                for (int ww = 0; ww < nw; ++ww) v += (double)red[ww * P + tid];
                accl[gh * 256 + tid] += v;
            }
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int i = tid; i < p.gmod * 256; i += 512) p.wg_acc[(int64_t)blockIdx.x * p.gmod * 256 + i] = accl[i];
#endif
}


// The several-K-steps form with MIXED operands (round 3): rows bf16 (the AdaLog-quantised attention probabilities, m * 2^-t), candidate
// columns fp8 e4m3 (q - z of a <= 4-bit uniform quantiser: exact small integers).  The candidate operand is what a launch streams
// (deit_small: 704 MB of bf16 per launch at 3.2 TB/s, written by the packer just before): as fp8 it is 256 instead of 448 bytes per
// column.  A lane's 16-byte LDS fragment holds 16 consecutive K values; v_cvt_scalef32_pk_bf16_fp8 (two values per instruction,
// exact) turns it into the B operands of two bf16 MFMAs, and the row fragments are loaded from global memory with the same
// lane -> K mapping:  MFMA m of 64-element K-step kt covers, for K half fkg,  K = 64 kt + 32 (m >> 1) + 16 fkg + 8 (m & 1) + 0..7.
template <int NJ, int NK>
__global__ __launch_bounds__(512, 2) void k_gemm_grpk8(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int NSG = 3, SB = 4, SBYTES = NK * SB * 32 * BK3;   // ring stages, blocks per stage (twice the bf16 form's: half the
                                                                  // barriers for the same 32 KiB stage), bytes per stage (fp8 columns)
    constexpr int RQ = NK * SB * 2, CQ = 4;                    // requests per stage (16 columns x 64 bytes each), requests per consumer
    constexpr int STG = NJ / SB > 0 ? NJ / SB : 1;             // stages per reference column
    constexpr int P = NJ * 32;
    static_assert(RQ > 7 * CQ, "the loader needs a share");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t* ring = lds;                                                        // [NSG][NK][64 columns][64 bytes]
    float* red = reinterpret_cast<float*>(lds + NSG * SBYTES);                  // [7 waves][P]
    double* accl = reinterpret_cast<double*>(lds + NSG * SBYTES + 7 * P * 4);   // [gmod][256]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fkg = lane >> 5;
    const int Kb = (int)p.Kb, KbA = (int)p.KbA;
    const int NB = p.N >> 5;
    const int CB = p.slab_R, NCH = p.slab_U;
    const int items = p.G * NCH;
    const int n_eff = p.N / P;
    for (int i = tid; i < p.gmod * 256; i += 512) accl[i] = 0.0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    const int lrow = lane >> 2, lslot16 = ((lane & 3) ^ ((lane >> 4) & 3)) << 4;
    int li = blockIdx.x, lst = 0, slot = 0, ahead = 0;
    auto stages_of = [&](int item) { const int c = item % NCH; return (min(CB, NB - c * CB) + SB - 1) / SB; };
    auto issue = [&]() {
        const int g = li / NCH, c = li - g * NCH;
        const int col0 = (c * CB + lst * SB) * 32;
        const int64_t left = (int64_t)(p.N - col0) * Kb;
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(p.B + (int64_t)g * p.sBg + (int64_t)col0 * Kb), 0,
                                                                            (int)(left < 0 ? 0 : min(left, (int64_t)0x7ffffffe)), 0x00020000);
        uint8_t* st = ring + slot * SBYTES;
        // request r: K-step r / (2 SB), columns 16 * (r % (2 SB)) .. + 15
        if (w == 7) {
#pragma unroll
            for (int r = 7 * CQ; r < RQ; ++r) STREAM_DMA(rb, st + r * 1024, ((r % (2 * SB)) * 16 + lrow) * Kb + lslot16, (r / (2 * SB)) * BK3);
        } else {
#pragma unroll
            for (int i = 0; i < CQ; ++i) {
                const int r = w * CQ + i;
                STREAM_DMA(rb, st + r * 1024, ((r % (2 * SB)) * 16 + lrow) * Kb + lslot16, (r / (2 * SB)) * BK3);
            }
        }
        slot = slot == NSG - 1 ? 0 : slot + 1;
        if (++lst == stages_of(li)) { lst = 0; li += gridDim.x; }
        ++ahead;
    };
    if (li < items) issue();
    if (li < items) issue();

    if (w == 7) {
        for (int item = blockIdx.x; item < items; item += gridDim.x) {
            const int ns = stages_of(item);
            for (int t = 0; t < ns; ++t) {
                static_assert(RQ - 7 * CQ == 4, "loader share");
                if (ahead >= 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // the following stage's four may be in flight
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                asm volatile("s_barrier" ::: "memory");
                --ahead;
                if (li < items) issue();
            }
            asm volatile("s_barrier" ::: "memory");
        }
    } else {
        const int row0 = w * 32;
        const bool rowblock_live = row0 < p.M;
        int st = 0;
        for (int item = blockIdx.x; item < items; item += gridDim.x) {
            const int g = item / NCH, c = item - g * NCH, gh = g % p.gmod;
            const int blk0 = c * CB, nblk = min(CB, NB - blk0), ns = (nblk + SB - 1) / SB;
            uint4 af[NK][4];
            {
                const bool ok = row0 + frow < p.M;
                const uint8_t* ar = p.A + (int64_t)g * p.sAg + (int64_t)min(row0 + frow, p.M - 1) * KbA;
#pragma unroll
                for (int kt = 0; kt < NK; ++kt)
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        af[kt][m] = *reinterpret_cast<const uint4*>(ar + kt * 128 + (m >> 1) * 64 + fkg * 32 + (m & 1) * 16);
                        if (!ok) af[kt][m] = make_uint4(0, 0, 0, 0);
                    }
            }
            float nal[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int ci = j * 32 + frow;
                nal[j] = -(p.sa[ci * p.sa_c + gh * p.sa_g] * p.sa_mul * p.sb[ci * p.sb_c + gh * p.sb_g]);
            }
            const uint32_t ref_bytes = (uint32_t)(((int64_t)(n_eff - 1) * p.ref_cs + p.M) * 4);
            const __amdgpu_buffer_rsrc_t rrg = __builtin_amdgcn_make_buffer_rsrc((void*)(p.ref + (int64_t)g * p.sRg), 0, (int)ref_bytes, 0x00020000);
            const bool full_rows = row0 + 32 <= p.M;
            int roff[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) roff[q] = min(row0 + 8 * q + 4 * fkg, p.M - 4) * 4;
            v2f cs2[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) cs2[j] = (v2f){0.0f, 0.0f};
            auto run = [&](auto full_tag) {
                constexpr bool FULL = decltype(full_tag)::value;
                auto load_ref = [&](int n, float4 (&r)[4]) {
                    const int coff = n < n_eff ? n * (int)p.ref_cs * 4 : 0x7ffffff0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const v4u uu = __builtin_amdgcn_raw_buffer_load_b128(rrg, roff[q], coff, 0);
                        r[q] = make_float4(__uint_as_float(uu.x), __uint_as_float(uu.y), __uint_as_float(uu.z), __uint_as_float(uu.w));
                    }
                };
                auto fix_ref = [&](float4 (&r)[4]) {
                    if (FULL) return;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int rr = row0 + 8 * q + 4 * fkg;
                        const float4 u = r[q];
                        const int sh = rr * 4 - roff[q];
                        const float e0 = sh == 0 ? u.x : sh == 4 ? u.y : sh == 8 ? u.z : u.w;
                        const float e1 = sh == 0 ? u.y : sh == 4 ? u.z : u.w;
                        const float e2 = sh == 0 ? u.z : u.w;
                        r[q] = make_float4(rr < p.M ? e0 : 0.f, rr + 1 < p.M ? e1 : 0.f, rr + 2 < p.M ? e2 : 0.f, rr + 3 < p.M ? u.w : 0.f);
                    }
                };
                int n = blk0 / NJ;
                float4 rc[4], rn[4];                           // current / next reference column
                load_ref(n, rc);
                load_ref(n + 1, rn);
                fix_ref(rc);
                for (int tg = 0; tg < ns; tg += STG) {
#pragma unroll
                    for (int s = 0; s < STG; ++s) {
                        // behind this wave's CQ requests of the stage: the next stage's CQ = 4 and the reference loads of the two
                        // stages in between (a stage is 4 blocks: at least 16 / 8 / 4 loads for NJ = 2 / 4 / 8)
                        if ((tg == 0 && s == 0) || ahead < 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        else if (NJ == 2) asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
                        else if (NJ == 4) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
                        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                        asm volatile("s_barrier" ::: "memory");
                        --ahead;
                        if (li < items) issue();
                        const uint8_t* cur = ring + st * SBYTES;
#pragma unroll
                        for (int b = 0; b < SB; ++b) {
                            const int j = (s * SB + b) % NJ;
                            v16f acc;
#pragma unroll
                            for (int kt = 0; kt < NK; ++kt) {
                                const uint8_t* ks = cur + kt * (SB * 32 * BK3);
                                const uint4 b0 = lds_frag(ks, swz3(b * 32 + frow, fkg)), b1 = lds_frag(ks, swz3(b * 32 + frow, 2 + fkg));
                                uint4 l0, h0, l1, h1;
                                fp8x16_bf16(b0, l0, h0);
                                fp8x16_bf16(b1, l1, h1);
                                if (kt == 0) acc = mma0<1>(af[0][0], l0); else mma<1>(af[kt][0], l0, acc);
                                mma<1>(af[kt][1], h0, acc);
                                mma<1>(af[kt][2], l1, acc);
                                mma<1>(af[kt][3], h1, acc);
                            }
                            const v2f na = {nal[j], nal[j]};
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const v2f tA = {acc[q * 4 + 0], acc[q * 4 + 1]}, tB = {acc[q * 4 + 2], acc[q * 4 + 3]};
                                const v2f rA = {rc[q].x, rc[q].y}, rB = {rc[q].z, rc[q].w};
                                const v2f dA = tA * na + rA, dB = tB * na + rB;
                                cs2[j] += dA * dA; cs2[j] += dB * dB;
                            }
                            if (j == NJ - 1) {                 // next block starts the next reference column
                                ++n;
#pragma unroll
                                for (int q = 0; q < 4; ++q) rc[q] = rn[q];
                                fix_ref(rc);
                                load_ref(n + 1, rn);
                            }
                        }
                        st = st == NSG - 1 ? 0 : st + 1;
                    }
                }
            };
            if (!rowblock_live) {
                for (int t = 0; t < ns; ++t) {
                    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
                    --ahead;
                    if (li < items) issue();
                    st = st == NSG - 1 ? 0 : st + 1;
                }
            } else if (full_rows) run(std::true_type{});
            else run(std::false_type{});
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                float cs = cs2[j].x + cs2[j].y;
                cs += __shfl_xor(cs, 32);
                if (fkg == 0) red[w * P + j * 32 + frow] = cs;
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (tid < P) {
                double v = 0.0;
                const int nw = min(7, (p.M + 31) / 32);
                for (int ww = 0; ww < nw; ++ww) v += (double)red[ww * P + tid];
                accl[gh * 256 + tid] += v;
            }
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int i = tid; i < p.gmod * 256; i += 512) p.wg_acc[(int64_t)blockIdx.x * p.gmod * 256 + i] = accl[i];
#endif
}


// Trimmed-K form of k_gemm_grpk8 (K <= 208: the 197 keys of a 224 x 224 ViT): rows of 13 sixteen-element slots instead of four
// 64-element K-steps -- fp8 candidate columns of Kb = 208 bytes, bf16 rows of KbA = 416 bytes -- so neither the packer, the
// L2 -> LDS path nor the matrix pipe touches the 48 all-zero K positions 208..255, and the MFMAs that only multiply zeros go.
//   * NKS MFMAs per 32 x 32 block, MFMA i with the operands of k_gemm_grpk8's MFMA i (kt = i / 4, m = i % 4), in the same
//     order: for K half fkg it covers K = 32 (i >> 1) + 16 fkg + 8 (i & 1) + 0..7.  MFMAs 0..11 cover K < 192; MFMA 12 covers
//     192..199 (fkg 0) and 208..215 (fkg 1: past the row, zeros in registers); MFMA 13 covers 200..207 and 216..223 (zeros).
//     So NKS = 13 holds every non-zero product of K <= 200 and NKS = 14 of K <= 208; the MFMAs left out multiply zeros by
//     zeros in k_gemm_grpk8 (an accumulator keeps its value; at most a zero changes sign, which d * d erases), and the
//     scores are bit-identical.  Epilogue, per-lane fp32 sums, wave order and the wg_acc layout are k_gemm_grpk8's.
//   * a 32-column block is one contiguous 6 656-byte run and a stage of SB = 4 blocks 26 624 bytes = 26 linear LDS-DMA requests
//     (64 lanes x 16 bytes); the LDS image equals the memory image.  The column stride is 13 slots -- odd, so the 32 columns
//     of a ds_read_b128 spread over the banks without a swizzle.  Lane (column, fkg) reads slots 2 pr + fkg, pr = 0..6
//     (slot 13 does not exist: zero).
//   * consumer w issues requests 3 w .. 3 w + 2, the loader wave requests 21..25.
template <int NJ, int NKS>
__global__ __launch_bounds__(512, 2) void k_gemm_grpk8t(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int NSL = 13, CBY = NSL * 16;                    // 16-byte slots / bytes of a column
    constexpr int NPR = (NKS + 1) / 2;                         // slot pairs (fkg 0 | fkg 1) = fragment reads per block and lane
    constexpr int NSG = 3, SB = 4, SBYTES = SB * 32 * CBY;     // ring stages, blocks per stage, bytes per stage
    constexpr int RQ = SBYTES / 1024, CQ = 3, LQ = RQ - 7 * CQ; // requests per stage / per consumer / of the loader
    constexpr int STG = NJ / SB > 0 ? NJ / SB : 1;             // stages per reference column
    constexpr int P = NJ * 32;
    static_assert(NKS == 13 || NKS == 14, "13 slots: MFMAs 12 and 13 are the last that can hold data");
    static_assert(SBYTES % 1024 == 0 && RQ == 26 && LQ == 5, "a stage is 26 whole requests: 7 x 3 + 5 for the loader");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t* ring = lds;                                                        // [NSG][128 columns][208 bytes]
    float* red = reinterpret_cast<float*>(lds + NSG * SBYTES);                  // [7 waves][P]
    double* accl = reinterpret_cast<double*>(lds + NSG * SBYTES + 7 * P * 4);   // [gmod][256]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fkg = lane >> 5;
    const int KbA = (int)p.KbA;
    const int NB = p.N >> 5;
    const int CB = p.slab_R, NCH = p.slab_U;
    const int items = p.G * NCH;
    const int n_eff = p.N / P;
    for (int i = tid; i < p.gmod * 256; i += 512) accl[i] = 0.0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    int li = blockIdx.x, lst = 0, slot = 0, ahead = 0;
    auto stages_of = [&](int item) { const int c = item % NCH; return (min(CB, NB - c * CB) + SB - 1) / SB; };
    auto issue = [&]() {
        const int g = li / NCH, c = li - g * NCH;
        const int col0 = (c * CB + lst * SB) * 32;
        const int64_t left = (int64_t)(p.N - col0) * CBY;      // bytes of the group from this stage on: past them a request reads zeros
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(p.B + (int64_t)g * p.sBg + (int64_t)col0 * CBY), 0,
                                                                            (int)(left < 0 ? 0 : min(left, (int64_t)0x7ffffffe)), 0x00020000);
        uint8_t* st = ring + slot * SBYTES;
        // request r: bytes 1024 r .. + 1023 of the stage (the whole offset in the VGPR: it is what the range check sees)
        if (w == 7) {
#pragma unroll
            for (int r = 7 * CQ; r < RQ; ++r) STREAM_DMA(rb, st + r * 1024, r * 1024 + lane * 16, 0);
        } else {
#pragma unroll
            for (int i = 0; i < CQ; ++i) {
                const int r = w * CQ + i;
                STREAM_DMA(rb, st + r * 1024, r * 1024 + lane * 16, 0);
            }
        }
        slot = slot == NSG - 1 ? 0 : slot + 1;
        if (++lst == stages_of(li)) { lst = 0; li += gridDim.x; }
        ++ahead;
    };
    if (li < items) issue();
    if (li < items) issue();

    if (w == 7) {
        for (int item = blockIdx.x; item < items; item += gridDim.x) {
            const int ns = stages_of(item);
            for (int t = 0; t < ns; ++t) {
                if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(LQ) : "memory");   // the following stage's LQ may be in flight
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                asm volatile("s_barrier" ::: "memory");
                --ahead;
                if (li < items) issue();
            }
            asm volatile("s_barrier" ::: "memory");
        }
    } else {
        const int row0 = w * 32;
        const bool rowblock_live = row0 < p.M;
        int st = 0;
        for (int item = blockIdx.x; item < items; item += gridDim.x) {
            const int g = item / NCH, c = item - g * NCH, gh = g % p.gmod;
            const int blk0 = c * CB, nblk = min(CB, NB - blk0), ns = (nblk + SB - 1) / SB;
            uint4 af[NKS];
            {
                const bool ok = row0 + frow < p.M;
                const uint8_t* ar = p.A + (int64_t)g * p.sAg + (int64_t)min(row0 + frow, p.M - 1) * KbA;
#pragma unroll
                for (int i = 0; i < NKS; ++i) {
                    const bool past = (i >> 1) == 6 && fkg == 1;              // K 208..: past the row
                    af[i] = *reinterpret_cast<const uint4*>(ar + (past ? 0 : (i >> 1) * 64 + fkg * 32) + (i & 1) * 16);
                    if (!ok || past) af[i] = make_uint4(0, 0, 0, 0);
                }
            }
            float nal[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int ci = j * 32 + frow;
                nal[j] = -(p.sa[ci * p.sa_c + gh * p.sa_g] * p.sa_mul * p.sb[ci * p.sb_c + gh * p.sb_g]);
            }
            const uint32_t ref_bytes = (uint32_t)(((int64_t)(n_eff - 1) * p.ref_cs + p.M) * 4);
            const __amdgpu_buffer_rsrc_t rrg = __builtin_amdgcn_make_buffer_rsrc((void*)(p.ref + (int64_t)g * p.sRg), 0, (int)ref_bytes, 0x00020000);
            const bool full_rows = row0 + 32 <= p.M;
            int roff[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) roff[q] = min(row0 + 8 * q + 4 * fkg, p.M - 4) * 4;
            v2f cs2[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) cs2[j] = (v2f){0.0f, 0.0f};
            auto run = [&](auto full_tag) {
                constexpr bool FULL = decltype(full_tag)::value;
                auto load_ref = [&](int n, float4 (&r)[4]) {
                    const int coff = n < n_eff ? n * (int)p.ref_cs * 4 : 0x7ffffff0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const v4u uu = __builtin_amdgcn_raw_buffer_load_b128(rrg, roff[q], coff, 0);
                        r[q] = make_float4(__uint_as_float(uu.x), __uint_as_float(uu.y), __uint_as_float(uu.z), __uint_as_float(uu.w));
                    }
                };
                auto fix_ref = [&](float4 (&r)[4]) {
                    if (FULL) return;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int rr = row0 + 8 * q + 4 * fkg;
                        const float4 u = r[q];
                        const int sh = rr * 4 - roff[q];
                        const float e0 = sh == 0 ? u.x : sh == 4 ? u.y : sh == 8 ? u.z : u.w;
                        const float e1 = sh == 0 ? u.y : sh == 4 ? u.z : u.w;
                        const float e2 = sh == 0 ? u.z : u.w;
                        r[q] = make_float4(rr < p.M ? e0 : 0.f, rr + 1 < p.M ? e1 : 0.f, rr + 2 < p.M ? e2 : 0.f, rr + 3 < p.M ? u.w : 0.f);
                    }
                };
                int n = blk0 / NJ;
                float4 rc[4], rn[4];                           // current / next reference column
                load_ref(n, rc);
                load_ref(n + 1, rn);
                fix_ref(rc);
                const int foff = frow * CBY + fkg * 16;        // this lane's slot 0 / 1 of column frow
                for (int tg = 0; tg < ns; tg += STG) {
#pragma unroll
                    for (int s = 0; s < STG; ++s) {
                        // behind this wave's CQ requests of the stage: the next stage's CQ and the reference loads of the two stages in
                        // between (a stage is 4 blocks: at least 16 / 8 / 4 loads for NJ = 2 / 4 / 8)
                        constexpr int BEHIND = CQ + (NJ == 2 ? 16 : NJ == 4 ? 8 : 4);
                        static_assert(BEHIND == (NJ == 2 ? 19 : NJ == 4 ? 11 : 7) && BEHIND < 64, "counted vmcnt of the consumers");
                        if ((tg == 0 && s == 0) || ahead < 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        else asm volatile("s_waitcnt vmcnt(%0)" :: "n"(BEHIND) : "memory");
                        asm volatile("s_barrier" ::: "memory");
                        --ahead;
                        if (li < items) issue();
                        const uint8_t* cur = ring + st * SBYTES;
#pragma unroll
                        for (int b = 0; b < SB; ++b) {
                            const int j = (s * SB + b) % NJ;
                            v16f acc;
#pragma unroll
                            for (int pr = 0; pr < NPR; ++pr) {
                                // the last pair's fkg 1 slot would be slot 13: read slot 12 (in range) and drop it
                                uint4 bq = lds_frag(cur, b * (32 * CBY) + foff + (pr == 6 ? 12 * 16 - fkg * 16 : pr * 32));
                                if (pr == 6 && fkg == 1) bq = make_uint4(0, 0, 0, 0);
                                uint4 lo, hi;
                                fp8x16_bf16(bq, lo, hi);
                                if (pr == 0) acc = mma0<1>(af[0], lo); else mma<1>(af[2 * pr], lo, acc);
                                if (2 * pr + 1 < NKS) mma<1>(af[2 * pr + 1], hi, acc);
                            }
                            const v2f na = {nal[j], nal[j]};
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const v2f tA = {acc[q * 4 + 0], acc[q * 4 + 1]}, tB = {acc[q * 4 + 2], acc[q * 4 + 3]};
                                const v2f rA = {rc[q].x, rc[q].y}, rB = {rc[q].z, rc[q].w};
                                const v2f dA = tA * na + rA, dB = tB * na + rB;
                                cs2[j] += dA * dA; cs2[j] += dB * dB;
                            }
                            if (j == NJ - 1) {                 // next block starts the next reference column
                                ++n;
#pragma unroll
                                for (int q = 0; q < 4; ++q) rc[q] = rn[q];
                                fix_ref(rc);
                                load_ref(n + 1, rn);
                            }
                        }
                        st = st == NSG - 1 ? 0 : st + 1;
                    }
                }
            };
            if (!rowblock_live) {
                for (int t = 0; t < ns; ++t) {
                    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
                    --ahead;
                    if (li < items) issue();
                    st = st == NSG - 1 ? 0 : st + 1;
                }
            } else if (full_rows) run(std::true_type{});
            else run(std::false_type{});
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                float cs = cs2[j].x + cs2[j].y;
                cs += __shfl_xor(cs, 32);
                if (fkg == 0) red[w * P + j * 32 + frow] = cs;
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (tid < P) {
                double v = 0.0;
                const int nw = min(7, (p.M + 31) / 32);
                for (int ww = 0; ww < nw; ++ww) v += (double)red[ww * P + tid];
                accl[gh * 256 + tid] += v;
            }
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int i = tid; i < p.gmod * 256; i += 512) p.wg_acc[(int64_t)blockIdx.x * p.gmod * 256 + i] = accl[i];
#endif
}


// GEN forms of the window / wave-private group kernels (round 4; uniform attention candidates, reference matmul.py:135-201): the
// candidate operand of a q.k^T search is P quantisations of the same [rows][K] fp32 tensor -- 1.1 GB packed and read back per
// launch for swin stage 0, where the window kernel is bound by exactly that stream.  Here a lane builds its MFMA operand fragment
// (16 consecutive K of candidate j * 32 + frow) from the fp32 row itself: t = x * (1 / s), rne, a tie-zone test per 16-value
// slot (|t - rne t| > tie -> the IEEE quotient decides, as the packer does), clamp, cvt -- the operand equals the packed one
// bit for bit.  The row slice is the same for the 32 lanes of a half wave (one broadcast 64-byte read, one row ahead).
struct GenCand { float s, inv, lo, hi; };
template <int DT>
__device__ __forceinline__ uint4 gen16(const float4 (&x4)[4], const GenCand& c, float tie) {
#pragma clang fp contract(off)
    constexpr float vbias = DT == 3 ? 0.0f : 128.0f;
    float xv[16], kq[16], dm = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { xv[4 * j] = x4[j].x; xv[4 * j + 1] = x4[j].y; xv[4 * j + 2] = x4[j].z; xv[4 * j + 3] = x4[j].w; }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const float t = xv[e] * c.inv;
        kq[e] = rintf(t);
        dm = fmaxf(dm, fabsf(t - kq[e]));
    }
    if (__builtin_expect(dm > tie, 0)) {
#pragma unroll
        for (int e = 0; e < 16; ++e) kq[e] = rintf(xv[e] / c.s);
    }
    uint32_t pk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float vb[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) vb[e] = __builtin_amdgcn_fmed3f(DT == 3 ? kq[4 * j + e] : kq[4 * j + e] + vbias, c.lo, c.hi);
        if constexpr (DT == 3) {
            const int lo2 = __builtin_amdgcn_cvt_pk_fp8_f32(vb[0], vb[1], 0, false);
            pk[j] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(vb[2], vb[3], lo2, true);
        } else {
            unsigned u = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) u = __builtin_amdgcn_cvt_pk_u8_f32(vb[e], e, u);
            pk[j] = u ^ 0x80808080u;
        }
    }
    return make_uint4(pk[0], pk[1], pk[2], pk[3]);
}
// candidate ci of head gh: scale from the epilogue's column factors (p.sb), zero point from gen_zp (same indexing)
template <int DT>
__device__ __forceinline__ GenCand gen_cand(const GemmArgs& p, int ci, int gh) {
    constexpr float vbias = DT == 3 ? 0.0f : 128.0f;
    const int64_t i = ci * p.sb_c + gh * p.sb_g;
    const float gs = p.sb[i], gz = rintf(p.gen_zp[i]);
    return {gs, __builtin_amdgcn_rcpf(gs), vbias - gz, vbias + (p.gen_qmax - gz)};
}

// ------------------------------------------------------------------------------------------------ window kernel
// Sixth form, for the attention searches of windowed models (swin: 49 queries x 49 keys x K = 32 per (window, head), 2 048
// to 8 192 such groups per launch): <= 64 rows, one 64-byte K-step, thousands of groups.  A launch is ALL epilogue (per
// 32 x 32 block one or two MFMAs against 32 outputs per lane), the streaming kernel spent it on tile set-up and staging at
// 0.03 of peak.  Here a WAVE owns a group and nothing is shared between waves, so there is no barrier in the loop:
//   * the group's row fragments (<= 2 row blocks) and its reference slice [keys][64 rows, zero padded] (wave-private LDS,
//     one coalesced pass) are loaded once per group;
//   * the candidate columns come straight from global memory into MFMA operand registers (a 32-column block is one
//     contiguous 2 KiB run), one reference column (P candidates = NJ blocks) ahead;
//   * the number of participating waves is a multiple of the heads per image, so a wave sees ONE head for the whole launch and
//     keeps its candidates' sums in registers (fp32 per group, fp64 across groups); the workgroup writes the
//     [workgroup][head][256] fp64 layout of k_gemm_stream at the end, in a fixed wave order.
template <int NJ, int DT, bool GEN = false>
__global__ __launch_bounds__(256, 2) void k_gemm_win(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int P = NJ * 32;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fkg = lane >> 5;
    const int Kb = (int)p.Kb;
    const int n_eff = p.N / P;
    const int RB = (p.M + 31) >> 5;                            // 1 or 2 row blocks
    const bool two_halves = p.Kvb > 32;                        // the second 32-byte half of the K-step holds data (rows of 32
                                                               // bytes -- K <= 32 packed without padding -- have none)
    float* refs = reinterpret_cast<float*>(lds) + w * (n_eff * 64);         // this wave's [n_eff][64]
    // the waves that take part are a multiple of the heads per image (the last W % gmod waves idle), so a wave's groups
    // wid, wid + W, ... all belong to ONE head
    const int W = ((int)gridDim.x * 4 / p.gmod) * p.gmod, wid = (int)blockIdx.x * 4 + w;
    const int gh = wid % p.gmod;
    double run[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) run[j] = 0.0;
    float nal[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int ci = j * 32 + frow;
        nal[j] = -(p.sa[ci * p.sa_c + gh * p.sa_g] * p.sa_mul * p.sb[ci * p.sb_c + gh * p.sb_g]);
    }
    GenCand gc[NJ];
    if constexpr (GEN) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) gc[j] = gen_cand<DT>(p, j * 32 + frow, gh);
    }
    for (int g = wid < W ? wid : p.G; g < p.G; g += W) {
        // ---- reference slice -> LDS (rows past M read as zero), row fragments -> registers
        const float* rg = p.ref + (int64_t)g * p.sRg;
        for (int n = 0; n < n_eff; ++n) refs[n * 64 + lane] = lane < p.M ? rg[(int64_t)n * p.ref_cs + lane] : 0.0f;
        uint4 a0[2], a1[2];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const int row = rb * 32 + frow;
            const bool ok = row < p.M;
            const uint8_t* ar = p.A + (int64_t)g * p.sAg + (int64_t)min(row, p.M - 1) * Kb;
            a0[rb] = *reinterpret_cast<const uint4*>(ar + fkg * 16);
            a1[rb] = two_halves ? *reinterpret_cast<const uint4*>(ar + 32 + fkg * 16) : make_uint4(0, 0, 0, 0);
            if (!ok) { a0[rb] = make_uint4(0, 0, 0, 0); a1[rb] = a0[rb]; }
        }
        const uint8_t* bg = GEN ? nullptr : p.B + (int64_t)g * p.sBg + (int64_t)frow * Kb + fkg * 16;
        auto load_cols = [&](int n, uint4 (&b0)[NJ], uint4 (&b1)[NJ]) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const uint8_t* bc = bg + (int64_t)(n * P + j * 32) * Kb;
                b0[j] = *reinterpret_cast<const uint4*>(bc);
                b1[j] = two_halves ? *reinterpret_cast<const uint4*>(bc + 32) : make_uint4(0, 0, 0, 0);
            }
        };
        // GEN: the lane's two 16-value slices of source row n (K elements fkg * 16 .. and 32 + fkg * 16 ..), one row ahead
        const float* xg = GEN ? p.gen_x + (int64_t)g * p.gen_sg + fkg * 16 : nullptr;
        const bool h0 = fkg * 16 < p.gen_K, h1 = 32 + fkg * 16 < p.gen_K;
        auto load_x = [&](int n, float4 (&x0)[4], float4 (&x1)[4]) {
            const float* xr = xg + (int64_t)n * p.gen_ldx;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                x0[q] = h0 ? *reinterpret_cast<const float4*>(xr + 4 * q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                x1[q] = h1 ? *reinterpret_cast<const float4*>(xr + 32 + 4 * q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        };
        uint4 bc0[NJ], bc1[NJ], bn0[NJ], bn1[NJ];
        float4 xc0[4], xc1[4], xn0[4], xn1[4];
        if constexpr (GEN) load_x(0, xc0, xc1); else load_cols(0, bc0, bc1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // this wave's reference slice is in LDS
        v2f cs2[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) cs2[j] = (v2f){0.0f, 0.0f};
        for (int n = 0; n < n_eff; ++n) {
            if constexpr (GEN) {
                if (n + 1 < n_eff) load_x(n + 1, xn0, xn1);
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    bc0[j] = h0 ? gen16<DT>(xc0, gc[j], p.gen_tie) : make_uint4(0, 0, 0, 0);
                    bc1[j] = h1 ? gen16<DT>(xc1, gc[j], p.gen_tie) : make_uint4(0, 0, 0, 0);
                }
            } else if (n + 1 < n_eff) load_cols(n + 1, bn0, bn1);
            float4 rr[2][4];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int q = 0; q < 4; ++q) rr[rb][q] = lds_f4(refs, n * 64 + rb * 32 + 8 * q + 4 * fkg);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const v2f na = {nal[j], nal[j]};
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    if (rb < RB) {
                        typename Acc<DT == 3 ? 1 : 0>::type acc;
                        if constexpr (DT == 3) {
                            v16f z_;
#pragma unroll
                            for (int e = 0; e < 16; ++e) z_[e] = 0.0f;
                            acc = mma_fp8x64(a0[rb], a1[rb], bc0[j], bc1[j], z_);
                        } else {
                            acc = mma0<0>(a0[rb], bc0[j]);
                            if (two_halves) mma<0>(a1[rb], bc1[j], acc);
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const v2f tA = {(float)acc[q * 4 + 0], (float)acc[q * 4 + 1]}, tB = {(float)acc[q * 4 + 2], (float)acc[q * 4 + 3]};
                            const v2f rA = {rr[rb][q].x, rr[rb][q].y}, rB = {rr[rb][q].z, rr[rb][q].w};
                            const v2f dA = tA * na + rA, dB = tB * na + rB;
                            cs2[j] += dA * dA; cs2[j] += dB * dB;
                        }
                    }
                }
            }
            if constexpr (GEN) {
#pragma unroll
                for (int q = 0; q < 4; ++q) { xc0[q] = xn0[q]; xc1[q] = xn1[q]; }
            } else {
#pragma unroll
                for (int j = 0; j < NJ; ++j) { bc0[j] = bn0[j]; bc1[j] = bn1[j]; }
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float cs = cs2[j].x + cs2[j].y;
            cs += __shfl_xor(cs, 32);
            run[j] += (double)cs;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // the slice is fully read before the next group overwrites it
    }
    // ---- [head][256] fp64 sums of this workgroup, waves added in a fixed order (the reference slices are dead now)
    double* accl = reinterpret_cast<double*>(lds);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int i = tid; i < p.gmod * 256; i += 256) accl[i] = 0.0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int ww = 0; ww < 4; ++ww) {
        if (w == ww && fkg == 0) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) accl[gh * 256 + j * 32 + frow] += run[j];
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    for (int i = tid; i < p.gmod * 256; i += 256) p.wg_acc[(int64_t)blockIdx.x * p.gmod * 256 + i] = accl[i];
#endif
}


// The window kernel with MIXED operands (round 3; swin's softmax.v weight search, matmul.py:173-201: 49 attention rows x 49 keys per
// (window, head), 32 x P candidate columns): rows bf16 (the AdaLog-quantised probabilities, 128-byte rows), candidate columns
// fp8 e4m3 (64-byte rows instead of the 128 bytes of a bf16 operand: these launches are bound by streaming 1.07 GB of candidates
// per 32 images).  Same organisation as k_gemm_win -- a wave owns a group, no barrier in the loop -- with the fp8 fragments
// converted to bf16 in registers (fp8x16_bf16: exact) and four bf16 MFMAs per (row block, column block); lane -> K mapping as in
// k_gemm_grpk8.
template <int NJ>
__global__ __launch_bounds__(256, 2) void k_gemm_winb(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int P = NJ * 32;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fkg = lane >> 5;
    const int Kb = (int)p.Kb, KbA = (int)p.KbA;              // 64-byte fp8 columns, 128-byte bf16 rows
    const int n_eff = p.N / P;
    const int RB = (p.M + 31) >> 5;                            // 1 or 2 row blocks
    float* refs = reinterpret_cast<float*>(lds) + w * (n_eff * 64);         // this wave's [n_eff][64]
    const int W = ((int)gridDim.x * 4 / p.gmod) * p.gmod, wid = (int)blockIdx.x * 4 + w;
    const int gh = wid % p.gmod;
    double run[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) run[j] = 0.0;
    float nal[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int ci = j * 32 + frow;
        nal[j] = -(p.sa[ci * p.sa_c + gh * p.sa_g] * p.sa_mul * p.sb[ci * p.sb_c + gh * p.sb_g]);
    }
    for (int g = wid < W ? wid : p.G; g < p.G; g += W) {
        const float* rg = p.ref + (int64_t)g * p.sRg;
        for (int n = 0; n < n_eff; ++n) refs[n * 64 + lane] = lane < p.M ? rg[(int64_t)n * p.ref_cs + lane] : 0.0f;
        uint4 af[2][4];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const int row = rb * 32 + frow;
            const bool ok = row < p.M;
            const uint8_t* ar = p.A + (int64_t)g * p.sAg + (int64_t)min(row, p.M - 1) * KbA;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                af[rb][m] = *reinterpret_cast<const uint4*>(ar + (m >> 1) * 64 + fkg * 32 + (m & 1) * 16);
                if (!ok) af[rb][m] = make_uint4(0, 0, 0, 0);
            }
        }
        const uint8_t* bg = p.B + (int64_t)g * p.sBg + (int64_t)frow * Kb + fkg * 16;
        auto load_cols = [&](int n, uint4 (&b0)[NJ], uint4 (&b1)[NJ]) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const uint8_t* bc = bg + (int64_t)(n * P + j * 32) * Kb;
                b0[j] = *reinterpret_cast<const uint4*>(bc);
                b1[j] = *reinterpret_cast<const uint4*>(bc + 32);
            }
        };
        uint4 bc0[NJ], bc1[NJ], bn0[NJ], bn1[NJ];
        load_cols(0, bc0, bc1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // this wave's reference slice is in LDS
        v2f cs2[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) cs2[j] = (v2f){0.0f, 0.0f};
        for (int n = 0; n < n_eff; ++n) {
            if (n + 1 < n_eff) load_cols(n + 1, bn0, bn1);
            float4 rr[2][4];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int q = 0; q < 4; ++q) rr[rb][q] = lds_f4(refs, n * 64 + rb * 32 + 8 * q + 4 * fkg);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const v2f na = {nal[j], nal[j]};
                uint4 l0, h0, l1, h1;
                fp8x16_bf16(bc0[j], l0, h0);
                fp8x16_bf16(bc1[j], l1, h1);
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    if (rb < RB) {
                        v16f acc = mma0<1>(af[rb][0], l0);
                        mma<1>(af[rb][1], h0, acc);
                        mma<1>(af[rb][2], l1, acc);
                        mma<1>(af[rb][3], h1, acc);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const v2f tA = {acc[q * 4 + 0], acc[q * 4 + 1]}, tB = {acc[q * 4 + 2], acc[q * 4 + 3]};
                            const v2f rA = {rr[rb][q].x, rr[rb][q].y}, rB = {rr[rb][q].z, rr[rb][q].w};
                            const v2f dA = tA * na + rA, dB = tB * na + rB;
                            cs2[j] += dA * dA; cs2[j] += dB * dB;
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) { bc0[j] = bn0[j]; bc1[j] = bn1[j]; }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float cs = cs2[j].x + cs2[j].y;
            cs += __shfl_xor(cs, 32);
            run[j] += (double)cs;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // the slice is fully read before the next group overwrites it
    }
    double* accl = reinterpret_cast<double*>(lds);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int i = tid; i < p.gmod * 256; i += 256) accl[i] = 0.0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int ww = 0; ww < 4; ++ww) {
        if (w == ww && fkg == 0) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) accl[gh * 256 + j * 32 + frow] += run[j];
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    for (int i = tid; i < p.gmod * 256; i += 256) p.wg_acc[(int64_t)blockIdx.x * p.gmod * 256 + i] = accl[i];
#endif
}


// Wave-private form of the q.k^T group kernel (round 3).  k_gemm_grp spends ~half of a launch in its stage barriers and DMA
// request issue (PMC: waves parked 60 % of the time, matrix pipe busy 17 %; halving the bytes of its sibling k_gemm_grpk8 did not
// change its time).  Here -- as in k_gemm_win -- nothing is shared between waves, so there is no barrier in the loop: a WAVE owns
// an item (group x chunk of reference columns), keeps the fragments of ALL row blocks of the group in registers (<= 7 x 2
// fragments: K is one 64-byte step), reads each 32-column candidate block straight from global memory into MFMA operand
// registers (one contiguous 2 KiB run, one block ahead) and multiplies it with every row block; the reference column (<= 224
// rows) is staged in wave-private LDS one column ahead.  Same [workgroup][head][256] fp64 output as the other forms.
template <int NJ, int DT, bool GEN = false>
__global__ __launch_bounds__(256, GEN ? 2 : 3) void k_gemm_grpw(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int P = NJ * 32, RBM = 7, RS = 224;              // candidates per column, row blocks at most, staged rows per column
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fkg = lane >> 5;
    const int Kb = (int)p.Kb;
    const int n_eff = p.N / P;
    const int RB = (p.M + 31) >> 5;
    float* refs = reinterpret_cast<float*>(lds) + w * (2 * RS);              // this wave's [2][RS]
    const int NCH = p.slab_U, CBc = p.slab_R;                  // chunks per group, reference columns per chunk
    const int items = p.G * NCH;
    // participating waves: a multiple of the heads per image (G % gmod == 0), so item wid + k W always belongs to head wid % gmod
    const int W = ((int)gridDim.x * 4 / p.gmod) * p.gmod, wid = (int)blockIdx.x * 4 + w;
    const int gh = wid % p.gmod;
    double run[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) run[j] = 0.0;
    float nal[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int ci = j * 32 + frow;
        nal[j] = -(p.sa[ci * p.sa_c + gh * p.sa_g] * p.sa_mul * p.sb[ci * p.sb_c + gh * p.sb_g]);
    }
    GenCand gc[NJ];
    if constexpr (GEN) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) gc[j] = gen_cand<DT>(p, j * 32 + frow, gh);
    }
    for (int idx = wid < W ? wid : items; idx < items; idx += W) {
        const int g = idx % p.G, c = idx / p.G;
        const int n_lo = c * CBc, n_hi = min(n_eff, n_lo + CBc);
        if (n_lo >= n_hi) continue;
        // ---- row fragments of the whole group (rows past M are zero)
        uint4 a0[RBM], a1[RBM];
#pragma unroll
        for (int rb = 0; rb < RBM; ++rb) {
            const int row = rb * 32 + frow;
            const bool ok = row < p.M;
            const uint8_t* ar = p.A + (int64_t)g * p.sAg + (int64_t)min(row, p.M - 1) * Kb;
            a0[rb] = *reinterpret_cast<const uint4*>(ar + fkg * 16);
            a1[rb] = *reinterpret_cast<const uint4*>(ar + 32 + fkg * 16);
            if (!ok) { a0[rb] = make_uint4(0, 0, 0, 0); a1[rb] = a0[rb]; }
        }
        // ---- reference column -> wave-private LDS: lane l stages rows l, l + 64, l + 128, l + 192 (zero past M)
        const float* rg = p.ref + (int64_t)g * p.sRg;
        auto ref_load = [&](int n, float (&v)[4]) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = lane + 64 * q;
                v[q] = (row < p.M && n < n_hi) ? rg[(int64_t)n * p.ref_cs + row] : 0.0f;
            }
        };
        auto ref_store = [&](int buf, const float (&v)[4]) {
#pragma unroll
            for (int q = 0; q < 4; ++q) if (lane + 64 * q < RS) refs[buf * RS + lane + 64 * q] = v[q];
        };
        float rv[4];
        ref_load(n_lo, rv);
        ref_store(0, rv);
        const uint8_t* bg = GEN ? nullptr : p.B + (int64_t)g * p.sBg + (int64_t)frow * Kb + fkg * 16;
        auto load_blk = [&](int blk, uint4& b0, uint4& b1) {      // blk = n * NJ + j: 32 consecutive candidate columns
            const uint8_t* bc = bg + (int64_t)blk * 32 * Kb;
            b0 = *reinterpret_cast<const uint4*>(bc);
            b1 = *reinterpret_cast<const uint4*>(bc + 32);
        };
        // GEN: the lane's two 16-value slices of source row n (K elements fkg * 16 .. and 32 + fkg * 16 ..), one row ahead
        const float* xg = GEN ? p.gen_x + (int64_t)g * p.gen_sg + fkg * 16 : nullptr;
        const bool h0 = fkg * 16 < p.gen_K, h1 = 32 + fkg * 16 < p.gen_K;
        auto load_x = [&](int n, float4 (&x0)[4], float4 (&x1)[4]) {
            const float* xr = xg + (int64_t)min(n, n_hi - 1) * p.gen_ldx;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                x0[q] = h0 ? *reinterpret_cast<const float4*>(xr + 4 * q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                x1[q] = h1 ? *reinterpret_cast<const float4*>(xr + 32 + 4 * q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        };
        // (two blocks ahead costs the third wave per SIMD: 59.6 against 50.8 ms per calibration)
        uint4 bc0, bc1, bn0, bn1;
        float4 xc0[4], xc1[4], xn0[4], xn1[4];
        if constexpr (GEN) load_x(n_lo, xc0, xc1); else load_blk(n_lo * NJ, bc0, bc1);
        v2f cs2[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) cs2[j] = (v2f){0.0f, 0.0f};
        for (int n = n_lo; n < n_hi; ++n) {
            const int buf = (n - n_lo) & 1;
            ref_load(n + 1, rv);                               // next column: global -> registers now, -> LDS after this column
            if constexpr (GEN) load_x(n + 1, xn0, xn1);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // this column's slice is in LDS (stored at the end of the last turn)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int nb = n * NJ + j + 1;
                if constexpr (GEN) {
                    bc0 = h0 ? gen16<DT>(xc0, gc[j], p.gen_tie) : make_uint4(0, 0, 0, 0);
                    bc1 = h1 ? gen16<DT>(xc1, gc[j], p.gen_tie) : make_uint4(0, 0, 0, 0);
                } else if (nb < n_hi * NJ) load_blk(nb, bn0, bn1);
                const v2f na = {nal[j], nal[j]};
#pragma unroll
                for (int rb = 0; rb < RBM; ++rb) {
                    if (rb < RB) {
                        typename Acc<DT == 3 ? 1 : 0>::type acc;
                        if constexpr (DT == 3) {
                            v16f z_;
#pragma unroll
                            for (int e = 0; e < 16; ++e) z_[e] = 0.0f;
                            acc = mma_fp8x64(a0[rb], a1[rb], bc0, bc1, z_);
                        } else {
                            acc = mma0<0>(a0[rb], bc0);
                            mma<0>(a1[rb], bc1, acc);
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float4 r4 = lds_f4(refs, buf * RS + rb * 32 + 8 * q + 4 * fkg);
                            const v2f tA = {(float)acc[q * 4 + 0], (float)acc[q * 4 + 1]}, tB = {(float)acc[q * 4 + 2], (float)acc[q * 4 + 3]};
                            const v2f rA = {r4.x, r4.y}, rB = {r4.z, r4.w};
                            const v2f dA = tA * na + rA, dB = tB * na + rB;
                            cs2[j] += dA * dA; cs2[j] += dB * dB;
                        }
                    }
                }
                if constexpr (!GEN) { bc0 = bn0; bc1 = bn1; }
            }
            if constexpr (GEN) {
#pragma unroll
                for (int q = 0; q < 4; ++q) { xc0[q] = xn0[q]; xc1[q] = xn1[q]; }
            }
            ref_store(buf ^ 1, rv);                            // (the other buffer was last read one column ago, by this wave)
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float cs = cs2[j].x + cs2[j].y;
            cs += __shfl_xor(cs, 32);
            run[j] += (double)cs;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    // ---- [head][256] fp64 sums of this workgroup, waves added in a fixed order (the reference slices are dead now)
    double* accl = reinterpret_cast<double*>(lds);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int i = tid; i < p.gmod * 256; i += 256) accl[i] = 0.0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int ww = 0; ww < 4; ++ww) {
        if (w == ww && fkg == 0) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) accl[gh * 256 + j * 32 + frow] += run[j];
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    for (int i = tid; i < p.gmod * 256; i += 256) p.wg_acc[(int64_t)blockIdx.x * p.gmod * 256 + i] = accl[i];
#endif
}


// ------------------------------------------------------------------------------------------------ log-base kernel
// softmax.v, log-base search of the post-softmax AdaLog quantiser (round 4; reference matmul.py:321-351): the P = 128 candidate
// bases q quantise the SAME probabilities, so the packed route wrote and read back 2.2 GB of bf16 candidates per launch (deit_small;
// pack 520 us + bf16 streaming kernel 650 us).  Here -- organised like k_gemm_grpw: a WAVE owns (group, chunk of <= 8 attention
// rows), nothing is shared between waves, no barrier in the loop --
//   * the fixed operand v^T (<= 64 rows x NKS 16-element K-steps, bf16) sits in registers for the whole item;
//   * the wave stages its rows in its own LDS once: L37 = fl(-fl(log2 p) * 37) with the CORRECTLY ROUNDED log2 (fp64 evaluation,
//     once per element instead of once per element and candidate) and the reference row.  The exact pipeline of the bin is then
//     t = fl(L37 / q), k = rne(t) (logarithm.py:94 as common.h adalog_k evaluates it): one division per element and candidate;
//   * a lane IS a candidate column: for candidate j * 32 + frow it turns its 8 values of a K-step into bins with
//     t = L37 * (1 / q) and, when a value of the slot is within 1e-4 of a tie, the IEEE quotient; clamps; reads the value
//     m * 2^-t (bf16 bits) from the [bin][candidate] table in LDS (conflict-free: the lane index is the candidate); bin nb is the
//     "masked" row (value 0: below the last bin, zero probabilities, K padding);
//   * bf16 MFMA against the register-resident rows, squared error against the reference row, fp64 sums per candidate in LDS.
// The operand equals the packer's bit for bit.  Same [workgroup][head][256] fp64 output as the other group kernels.
constexpr int AVQ_ROWS = 8;                                    // attention rows per item at most (LDS: rows staged once per item)
template <int NJ, int NKS, int RB>
__global__ __launch_bounds__(256, 2) void k_gemm_avq(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int P = NJ * 32, KP = NKS * 16;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fkg = lane >> 5;
    const int n_eff = p.N / P;
    const int K = p.gen_K, nb = p.gen_nb;                       // (RB: row blocks of the fixed operand, (M + 31) / 32)
    // LDS: the value table [nb + 1][P] dwords | per wave: AVQ_ROWS x (L37 row [KP] | reference row [64]) | fp64 sums [NJ][64]
    uint32_t* lut = reinterpret_cast<uint32_t*>(lds);
    const int lut_words = ((nb + 1) * P + 3) & ~3;
    constexpr int ROW = KP + 64, WAVE_F = AVQ_ROWS * ROW + NJ * 64 * 2;
    float* mine = reinterpret_cast<float*>(lds) + lut_words + w * WAVE_F;
    double* sums = reinterpret_cast<double*>(mine + AVQ_ROWS * ROW);
    for (int i = tid; i < (nb + 1) * P; i += 256) lut[i] = p.gen_lut[i];
#pragma unroll
    for (int j = 0; j < NJ; ++j) sums[j * 64 + lane] = 0.0;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const int NCH = p.slab_U, CBc = p.slab_R;
    const int items = p.G * NCH;
    const int W = ((int)gridDim.x * 4 / p.gmod) * p.gmod, wid = (int)blockIdx.x * 4 + w;
    const int gh = wid % p.gmod;
    const float nbf = (float)nb;
    for (int idx = wid < W ? wid : items; idx < items; idx += W) {
        const int g = idx % p.G, c = idx / p.G;
        const int n_lo = c * CBc, n_hi = min(n_eff, n_lo + CBc);
        if (n_lo >= n_hi) continue;
        // ---- fixed rows (v^T) of the group: RB x NKS fragments of 8 bf16
        uint4 af[RB][NKS];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const int row = rb * 32 + frow;
            const uint8_t* ar = p.A + (int64_t)g * p.sAg + (int64_t)min(row, p.M - 1) * p.Kb + fkg * 16;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks)
                af[rb][ks] = row < p.M ? *reinterpret_cast<const uint4*>(ar + ks * 32) : make_uint4(0, 0, 0, 0);
        }
        // ---- the item's rows -> LDS: L37 (lane l takes elements l, l + 64, ...) and the reference row (lane = row of v^T)
        const float* xg = p.gen_x + (int64_t)g * p.gen_sg;
        const float* rg = p.ref + (int64_t)g * p.sRg;
        for (int n = n_lo; n < n_hi; ++n) {
            float* r = mine + (n - n_lo) * ROW;
#pragma unroll
            for (int i = 0; i < (KP + 63) / 64; ++i) {
                const int e = lane + 64 * i;
                if (e < KP) {
                    const float u = e < K ? xg[(int64_t)n * p.gen_ldx + e] : 0.0f;
                    // u = 0 (masked code, K padding): L37 = +inf -> t = +inf -> bin nb
                    r[e] = u > 0.0f ? (-(float)log2((double)u)) * 37.0f : __builtin_inff();
                }
            }
            r[KP + lane] = lane < p.M ? rg[(int64_t)n * p.ref_cs + lane] : 0.0f;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 1
        for (int j = 0; j < NJ; ++j) {
            const int ci = j * 32 + frow;
            const float qf = p.gen_q[ci], rq = __builtin_amdgcn_rcpf(qf);
            const float nal = -(p.sa[ci * p.sa_c + gh * p.sa_g] * p.sa_mul * p.sb[ci * p.sb_c + gh * p.sb_g]);
            const v2f na = {nal, nal};
            const uint32_t* lj = lut + ci;
            v2f cs2 = {0.0f, 0.0f};
#pragma unroll 1
            for (int n = n_lo; n < n_hi; ++n) {
                const float* Lr = mine + (n - n_lo) * ROW;
                // phase 1: the candidate's operand fragments of this row (the tie branch sits here, away from the accumulators)
                uint4 bfrag[NKS];
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const float4 l0 = lds_f4(Lr, ks * 16 + fkg * 8), l1 = lds_f4(Lr, ks * 16 + fkg * 8 + 4);
                    const float Lv[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
                    float kk[8], dm = 0.0f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float t = Lv[e] * rq;
                        kk[e] = rintf(t);
                        dm = fmaxf(dm, fabsf(t - kk[e]));               // (t = +inf: t - k is NaN, fmaxf drops it)
                    }
                    if (__builtin_expect(dm > 0.4999f, 0)) {            // a value of this slot is near a tie: the IEEE quotient decides
#pragma unroll
                        for (int e = 0; e < 8; ++e) kk[e] = rintf(Lv[e] / qf);
                    }
                    uint32_t v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = lj[(int)__builtin_amdgcn_fmed3f(kk[e], 0.0f, nbf) * P];
                    bfrag[ks] = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
                }
                // phase 2: the products
                v16f acc[RB];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[rb][e] = 0.0f;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) mma<1>(af[rb][ks], bfrag[ks], acc[rb]);
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 r4 = lds_f4(Lr, KP + rb * 32 + 8 * q + 4 * fkg);
                        const v2f tA = {acc[rb][q * 4 + 0], acc[rb][q * 4 + 1]}, tB = {acc[rb][q * 4 + 2], acc[rb][q * 4 + 3]};
                        const v2f rA = {r4.x, r4.y}, rB = {r4.z, r4.w};
                        const v2f dA = tA * na + rA, dB = tB * na + rB;
                        cs2 += dA * dA; cs2 += dB * dB;
                    }
                }
            }
            sums[j * 64 + lane] += (double)(cs2.x + cs2.y);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // the rows are fully read before the next item overwrites them
    }
    // ---- [head][256] fp64 sums of this workgroup: the two K halves of a candidate, then the waves in a fixed order
    double run[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) run[j] = sums[j * 64 + frow] + sums[j * 64 + 32 + frow];
    double* accl = reinterpret_cast<double*>(lds);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int i = tid; i < p.gmod * 256; i += 256) accl[i] = 0.0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int ww = 0; ww < 4; ++ww) {
        if (w == ww && fkg == 0) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) accl[gh * 256 + j * 32 + frow] += run[j];
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    for (int i = tid; i < p.gmod * 256; i += 256) p.wg_acc[(int64_t)blockIdx.x * p.gmod * 256 + i] = accl[i];
#endif
}
