// Part of gemm_score.hip (one translation unit, included inside its anonymous namespace): general kernel (C > 1), large-tile kernel (C = 1) and its LDS-DMA pipelined form.
template <int DT, bool STORE>
__global__ __launch_bounds__(256, 2) void k_gemm_score(GemmArgs p) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * (BM + BN) * BKB];
    __shared__ float red[2][2][2][32];
    __shared__ float colv[128];
    uint8_t* As = lds;
    uint8_t* Bs = lds + 2 * BM * BKB;

    // ---- XCD-aware bijective block remap: consecutive logical tiles (same A tile, neighbouring n) share an XCD/L2
    const unsigned nwg = gridDim.x, bid = blockIdx.x;
    const unsigned q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    const unsigned lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    // Tile order = which operand stays hot in the XCD's 4 MiB L2 while its neighbours run:
    //   1 (activation / matmul searches): the n-tiles of one (candidate, m-tile) share the candidate's A tile, and all
    //     candidates of one m-tile share the fp32 reference rows and the fixed operand;
    //   2 (weight searches, columns = (out-channel, candidate)): all m-tiles of one column tile share its packed weights.
    unsigned t = lid;
    int nt, mt, g, c;
    if (p.order == 1) { nt = t % p.NT; t /= p.NT; c = t % p.C; t /= p.C; mt = t % p.MT; g = t / p.MT; }
    else if (p.order == 2) { mt = t % p.MT; t /= p.MT; nt = t % p.NT; t /= p.NT; c = t % p.C; g = t / p.C; }
    else { nt = t % p.NT; t /= p.NT; mt = t % p.MT; t /= p.MT; g = t % p.G; c = t / p.G; }
    const int gh = g % p.gmod;
    const int m0 = mt * BM, n0 = nt * BN;

    const uint8_t* Ag = p.A + c * p.sAc + g * p.sAg;
    const uint8_t* Bg = p.B + c * p.sBc + g * p.sBg;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    // global->LDS staging: thread loads rows (tid>>2) and (tid>>2)+64, 16-byte slot tid&3
    const int lrow = tid >> 2, lslot = tid & 3;
    int ar0 = m0 + lrow, ar1 = m0 + lrow + 64, br0 = n0 + lrow, br1 = n0 + lrow + 64;
    ar0 = ar0 < p.M ? ar0 : p.M - 1; ar1 = ar1 < p.M ? ar1 : p.M - 1;      // edge rows: clamp, masked in epilogue
    br0 = br0 < p.N ? br0 : p.N - 1; br1 = br1 < p.N ? br1 : p.N - 1;
    const uint4* ga0 = reinterpret_cast<const uint4*>(Ag + (int64_t)ar0 * p.Kb) + lslot;
    const uint4* ga1 = reinterpret_cast<const uint4*>(Ag + (int64_t)ar1 * p.Kb) + lslot;
    const uint4* gb0 = reinterpret_cast<const uint4*>(Bg + (int64_t)br0 * p.Kb) + lslot;
    const uint4* gb1 = reinterpret_cast<const uint4*>(Bg + (int64_t)br1 * p.Kb) + lslot;
    const int so0 = swz(lrow, lslot), so1 = swz(lrow + 64, lslot);

    typename Acc<DT>::type acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

    const int nk = (int)(p.Kb / BKB);
    uint4 ra0 = ga0[0], ra1 = ga1[0], rb0 = gb0[0], rb1 = gb1[0];
    *reinterpret_cast<uint4*>(As + so0) = ra0; *reinterpret_cast<uint4*>(As + so1) = ra1;
    *reinterpret_cast<uint4*>(Bs + so0) = rb0; *reinterpret_cast<uint4*>(Bs + so1) = rb1;
    __syncthreads();

    const int frow = lane & 31, fkg = lane >> 5;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) {
            const int o = (kt + 1) * (BKB / 16);
            ra0 = ga0[o]; ra1 = ga1[o]; rb0 = gb0[o]; rb1 = gb1[o];
        }
        const uint8_t* Ac = As + cur * BM * BKB;
        const uint8_t* Bc = Bs + cur * BN * BKB;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint4 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const uint4*>(Ac + swz(wr * 64 + i * 32 + frow, ks * 2 + fkg));
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const uint4*>(Bc + swz(wc * 64 + j * 32 + frow, ks * 2 + fkg));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mma<DT>(af[i], bf[j], acc[i][j]);
        }
        if (kt + 1 < nk) {
            uint8_t* An = As + (cur ^ 1) * BM * BKB;
            uint8_t* Bn = Bs + (cur ^ 1) * BN * BKB;
            *reinterpret_cast<uint4*>(An + so0) = ra0; *reinterpret_cast<uint4*>(An + so1) = ra1;
            *reinterpret_cast<uint4*>(Bn + so0) = rb0; *reinterpret_cast<uint4*>(Bn + so1) = rb1;
        }
        __syncthreads();
    }

    // ---- epilogue: out = acc * (sa*sb) + bias; squared error against ref; column sums over the tile's rows.
    // With ref_div > 1 a GEMM column encodes (output channel n = col / ref_div, candidate = col % ref_div): the 128
    // candidates of one channel sit in one tile and share ONE reference column (weight searches).
    // Branch-free: edge rows/columns are clamped for addressing and weighted 0; 32-bit offsets inside a group.
    const float* refg = p.ref ? p.ref + (int64_t)g * p.sRg : nullptr;
    float* outg = STORE ? p.out + (int64_t)c * p.sOc + (int64_t)g * p.sOg : nullptr;
    const int ldr = (int)p.ldr, rcs = (int)p.ref_cs, ldo = (int)p.ldo;
    const bool interior = (m0 + BM <= p.M) && (n0 + BN <= p.N);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wc * 64 + j * 32 + frow;
        const bool cv = col < p.N;
        const int colc = cv ? col : p.N - 1;
        const int ci = p.ref_div > 1 ? colc % p.ref_div : c;
        const int ni = p.ref_div > 1 ? colc / p.ref_div : colc;
        const float alpha = p.sa[ci * p.sa_c + gh * p.sa_g] * p.sa_mul * p.sb[ci * p.sb_c + gh * p.sb_g + ni * p.sb_n];
        const float beta = p.bias ? p.bias[ci * p.bi_c + gh * p.bi_g + ni * p.bi_n] : 0.0f;
        const int rc0 = ni * rcs;
        float csum = 0.0f;
        if (interior) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int rb = m0 + wr * 64 + i * 32 + 4 * fkg;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = rb + (r & 3) + 8 * (r >> 2);
                    const float o = (float)acc[i][j][r] * alpha + beta;
                    if (STORE) outg[row * ldo + col] = o;
                    if (refg) {
                        const float e = refg[row * ldr + rc0] - o;
                        csum += e * e;
                    }
                }
            }
        } else {
            const float cm = cv ? 1.0f : 0.0f;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int rb = m0 + wr * 64 + i * 32 + 4 * fkg;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = rb + (r & 3) + 8 * (r >> 2);
                    const bool rv = row < p.M;
                    const int rowc = rv ? row : p.M - 1;
                    const float o = (float)acc[i][j][r] * alpha + beta;
                    if (STORE) { if (rv && cv) outg[rowc * ldo + col] = o; }
                    if (refg) {
                        const float e = refg[rowc * ldr + rc0] - o;
                        csum += (e * e) * (rv ? cm : 0.0f);
                    }
                }
            }
        }
        csum += __shfl_xor(csum, 32);
        if (fkg == 0) red[wr][wc][j][frow] = csum;
    }
    if (p.partial) {
        __syncthreads();
        float v = 0.0f;
        int col = 0;
        if (tid < 128) {
            const int cwc = tid >> 6, cj = (tid >> 5) & 1, cl = tid & 31;
            col = n0 + cwc * 64 + cj * 32 + cl;
            v = red[0][cwc][cj][cl] + red[1][cwc][cj][cl];
        }
        if (p.reduce_cols) {                       // fixed-order tile total: LDS, then one wave's xor tree
            if (tid < 128) colv[tid] = v;
            __syncthreads();
            if (tid < 64) {
                float t2 = colv[tid] + colv[tid + 64];
#pragma unroll
                for (int sft = 32; sft > 0; sft >>= 1) t2 += __shfl_xor(t2, sft);
                if (tid == 0) p.partial[(((int64_t)c * p.G + g) * p.MT + mt) * p.Npad + nt] = t2;
            }
        } else if (tid < 128) {
            if (p.ref_div > 1) {
                if (col < p.N)
                    p.partial[((((int64_t)g) * p.MT + mt) * p.Npad + col / p.ref_div) * p.ref_div + col % p.ref_div] = v;
            } else if (col < p.Npad) {
                p.partial[(((int64_t)c * p.G + g) * p.MT + mt) * p.Npad + col] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ large-tile kernel
// Second-generation scoring kernel, used whenever the candidates sit in the GEMM's column axis (every search) or there
// is a single problem per group (quant_forward).  Per 512-thread workgroup (8 waves as 2 x 4): (64*TM) x 256 output tile,
// K-step = 128 BYTES so that every staged row is one full 128-byte cache line (the 64-byte steps of the first kernel
// fetched each line twice and left it latency-bound: MFMA 13 % busy, 64 % of wave cycles parked, profiles/r01_pmc_*).
// Per wave (32*TM) x 64 = TM x 2 MFMA 32x32 tiles; operand bytes per MAC are half those of the 128 x 128 tile.
// One LDS stage (<= 64 KiB -> 2 workgroups per CU) + register prefetch of the next K-step.
constexpr int BN2 = 256, BK2 = 128;

__device__ __forceinline__ int swz2(int row, int slot) { return row * BK2 + ((slot ^ ((row >> 1) & 7)) << 4); }

// Epilogue of the large-tile kernel, specialised at compile time so the unrolled body is branch-free:
//   STORE: write out (quant_forward) / else: squared error against ref;  EDGE: tile touches the M or N boundary;
//   ROWS: per-row scale and bias present.
template <int DT, int TM, bool STORE, bool EDGE, bool ROWS, bool ADD = false, bool ROWMAP = false>
__device__ __forceinline__ void epilogue2(const GemmArgs& p, typename Acc<DT>::type (&acc)[TM][2], int g, int gh, int m0,
                                          int n0, int wr, int wc, int frow, int fkg, float* red) {
    constexpr int BM2 = 64 * TM;
    const float* refg = STORE ? nullptr : p.ref + (int64_t)g * p.sRg;
    // ADD (quant_forward extras, adalog_gemm_out_ex): two-level output groups and the residual stream
    const int64_t ogo = !STORE ? 0 : ((ADD && p.out_gi > 0) ? (int64_t)(g % p.out_gi) * p.sOg + (int64_t)(g / p.out_gi) * p.sOo : (int64_t)g * p.sOg);
    float* outg = STORE ? p.out + ogo : nullptr;
    const float* addg = (STORE && ADD && p.addend) ? p.addend + ogo : nullptr;
    const int ldr = (int)p.ldr, rcs = (int)p.ref_cs, ldo = (int)p.ldo;
    // ROWMAP: the row of out / addend that GEMM row `row` lands on (the row scatter of adalog_gemm_out_gen_rows)
    [[maybe_unused]] auto orow = [&](int row) {
        if constexpr (ROWMAP) {
            if (p.o_rows) { const int im = row / p.row_period; return p.o_rows[row - im * p.row_period] + im * p.row_period; }
        }
        return row;
    };
    float alpha[2], beta[2], cm[2], csum[2] = {0.0f, 0.0f};
    int rc0[2], colj[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wc * 64 + j * 32 + frow;
        const bool cv = !EDGE || col < p.N;
        colj[j] = col;
        const int colc = cv ? col : p.N - 1;
        const int ci = p.ref_div > 1 ? colc % p.ref_div : 0;
        const int ni = p.ref_div > 1 ? colc / p.ref_div : colc;
        alpha[j] = p.sa[ci * p.sa_c + gh * p.sa_g] * p.sa_mul * p.sb[ci * p.sb_c + gh * p.sb_g + ni * p.sb_n];
        beta[j] = p.bias ? p.bias[ci * p.bi_c + gh * p.bi_g + ni * p.bi_n] : 0.0f;
        rc0[j] = ni * rcs;
        cm[j] = cv ? 1.0f : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int rb0 = m0 + wr * (BM2 / 2) + i * 32 + 4 * fkg;
        // the residual stream (STORE, addend): the 32 values of this row block are requested back to back BEFORE the first store --
        // out and addend may alias as far as the compiler knows, so a load placed after a store would wait for it (a chain of 32
        // memory round trips per row block: the projection's launch went 23 -> 29 us with the loads inside the store loop)
        float av[(STORE && ADD) ? 16 : 1][2];
        if (STORE && ADD) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rb0 + (r & 3) + 8 * (r >> 2);
                const bool rv = !EDGE || row < p.M;
                const int ro = ROWMAP ? (rv ? orow(row) : 0) : row;
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    av[r][j] = (addg && rv && (!EDGE || cm[j] != 0.0f)) ? addg[ro * ldo + colj[j]] : 0.0f;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rb0 + (r & 3) + 8 * (r >> 2);
            if (!EDGE || row < p.M) {                   // edge tiles (rare) predicate whole rows; interior tiles have no branch
                [[maybe_unused]] const int ro = ROWMAP ? orow(row) : row;
                float rs = 1.0f, rbv = 0.0f;
                if (ROWS) { rs = p.row_scale[row]; rbv = p.row_bias[row]; }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float o = (float)acc[i][j][r] * alpha[j];
                    if (ROWS) o = o * rs + rbv;
                    o += beta[j];
                    if (STORE) {
                        if (!EDGE || cm[j] != 0.0f) {
                            if (ADD) { if (addg) o += av[r][j]; }
                            outg[(ROWMAP ? ro : row) * ldo + colj[j]] = o;
                        }
                    } else {
                        const float e = refg[row * ldr + rc0[j]] - o;
                        csum[j] += EDGE ? (e * e) * cm[j] : e * e;
                    }
                }
            }
            if ((r & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (!STORE) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float cs = csum[j];
            cs += __shfl_xor(cs, 32);
            if (fkg == 0) red[((wr * 4 + wc) * 2 + j) * 32 + frow] = cs;
        }
    }
}

// Scoring epilogue with the reference slice staged through LDS (candidates-in-columns layout, rows contiguous in ref:
// ldr == 1).  The tile needs only (256 / ref_div) reference columns x BM2 rows (1-4 KiB instead of BM2 x 256 values):
// they are fetched with one coalesced pass, and each thread then reads four consecutive rows per ds_read_b128.
template <int DT, int TM, bool EDGE, bool ROWS>
__device__ __forceinline__ void epilogue_lds(const GemmArgs& p, typename Acc<DT>::type (&acc)[TM][2], int g, int gh, int m0,
                                             int n0, int wr, int wc, int frow, int fkg, float* red, float* stage) {
    constexpr int BM2 = 64 * TM;
    const float* refg = p.ref + (int64_t)g * p.sRg;
    const int rcs = (int)p.ref_cs;
    const int nref = BN2 / p.ref_div;                       // reference columns touched by this tile (<= 8)
    const int ni0 = n0 / p.ref_div;
    const int nvalid = (p.N / p.ref_div) - ni0;              // reference columns that exist
    float* refs = stage;                                     // [nref][BM2]
    float* rsc = stage + 8 * BM2;                            // [BM2]
    float* rbi = rsc + BM2;
    const int tid = threadIdx.x;
    for (int e = tid; e < nref * BM2; e += 512) {
        const int nl = e / BM2, rl = e - nl * BM2;
        const int row = m0 + rl;
        float v = 0.0f;
        if ((!EDGE || row < p.M) && nl < nvalid) v = refg[row + (ni0 + nl) * rcs];
        refs[e] = v;
    }
    if (ROWS) {
        for (int e = tid; e < BM2; e += 512) {
            const int row = m0 + e;
            const bool ok = !EDGE || row < p.M;
            rsc[e] = ok ? p.row_scale[row] : 0.0f;
            rbi[e] = ok ? p.row_bias[row] : 0.0f;
        }
    }
    __syncthreads();
    float alpha[2], beta[2], cm[2], csum[2] = {0.0f, 0.0f};
    const float* rj[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wc * 64 + j * 32 + frow;
        const bool cv = !EDGE || col < p.N;
        const int colc = cv ? col : p.N - 1;
        const int ci = colc % p.ref_div, ni = colc / p.ref_div;
        alpha[j] = p.sa[ci * p.sa_c + gh * p.sa_g] * p.sa_mul * p.sb[ci * p.sb_c + gh * p.sb_g + ni * p.sb_n];
        beta[j] = p.bias ? p.bias[ci * p.bi_c + gh * p.bi_g + ni * p.bi_n] : 0.0f;
        cm[j] = cv ? 1.0f : 0.0f;
        rj[j] = refs + (ni - ni0) * BM2;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int rl = wr * (BM2 / 2) + i * 32 + 4 * fkg + 8 * q4;          // 4 consecutive rows rl .. rl+3
            const float4 r0 = *reinterpret_cast<const float4*>(rj[0] + rl);
            const float4 r1 = *reinterpret_cast<const float4*>(rj[1] + rl);
            float4 s4 = make_float4(1.f, 1.f, 1.f, 1.f), b4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ROWS) { s4 = *reinterpret_cast<const float4*>(rsc + rl); b4 = *reinterpret_cast<const float4*>(rbi + rl); }
            const float rr0[4] = {r0.x, r0.y, r0.z, r0.w}, rr1[4] = {r1.x, r1.y, r1.z, r1.w};
            const float ss[4] = {s4.x, s4.y, s4.z, s4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = q4 * 4 + k;
                float w = 1.0f;
                if (EDGE) w = (m0 + rl + k < p.M) ? 1.0f : 0.0f;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float o = (float)acc[i][j][r] * alpha[j];
                    if (ROWS) o = o * ss[k] + bb[k];
                    o += beta[j];
                    const float e = (j == 0 ? rr0[k] : rr1[k]) - o;
                    csum[j] += EDGE ? (e * e) * (w * cm[j]) : e * e;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float cs = csum[j];
        cs += __shfl_xor(cs, 32);
        if (fkg == 0) red[((wr * 4 + wc) * 2 + j) * 32 + frow] = cs;
    }
}

// GENA (round 6, quant_forward): the A operand is NOT read packed -- a thread quantises its 16 values of each of its rows straight
// from the fp32 activation (p.gen_x, rows p.gen_ldx apart, groups p.gen_sg apart; K valid = p.gen_K, a multiple of 16) with the
// per-tensor / per-head uniform quantiser (p.gen_scale / p.gen_zp [g % gmod * p.gen_sn]) on the way from its registers to LDS: the
// packer's arithmetic (reciprocal multiply, IEEE quotient inside the tie zone, clamp, biased u8 conversion), so the int8 image in
// LDS equals adalog_pack_uniform's bit for bit and the separate pack launch of the activation disappears (reference
// quant_layers/linear.py:46-51: q_a(x) inside the layer's forward).  int8 only (DT == 0).
//
// ROWMAP (quant_forward of a Swin block, adalog_gemm_out_gen_rows): the generated A rows are gathered and the STORE epilogue's rows
// scattered through the maps of GemmArgs (a_rows / o_rows, period row_period) -- roll + window partition in front of qkv, window
// reverse + roll back + the residual add behind proj.
template <int DT, int TM, bool STORE, bool GENA = false, bool ADD = false, bool ROWMAP = false>
__global__ __launch_bounds__(512, 2) void k_gemm_cand(GemmArgs p) {
    static_assert(!ADD || STORE, "the epilogue extras belong to the STORE form");
    static_assert(!ROWMAP || (GENA && STORE), "the row maps belong to the generated-A STORE form");
    static_assert(!GENA || (DT == 0 && TM <= 2), "the generated A operand: int8, at most two row blocks per thread");
    constexpr int BM2 = 64 * TM;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t* As = smem;
    uint8_t* Bs = smem + BM2 * BK2;
    float* red = reinterpret_cast<float*>(smem + (BM2 + BN2) * BK2);       // [2][4][2][32] then colv[256]
    float* colv = red + 512;

    const unsigned nwg = gridDim.x, bid = blockIdx.x;
    const unsigned q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    const unsigned lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    unsigned t = lid;
    int nt, mt, g;
    if (p.order == 2) { mt = t % p.MT; t /= p.MT; nt = t % p.NT; g = t / p.NT; }
    else { nt = t % p.NT; t /= p.NT; mt = t % p.MT; g = t / p.MT; }
    const int gh = g % p.gmod;
    const int m0 = mt * BM2, n0 = nt * BN2;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 2, wc = w & 3;
    const int lrow = tid >> 3, lslot = tid & 7;
    // per-thread global source addresses (clamped rows at the edges) and swizzled LDS destinations
    const uint8_t* Ab = p.A + g * p.sAg + lslot * 16;
    const uint8_t* Bb = p.B + g * p.sBg + lslot * 16;
    int64_t oa0, oa1, oa2, oa3, ob0, ob1, ob2, ob3;
    {
        auto rowoff = [&](int base, int lim) { int r = base < lim ? base : lim - 1; return (int64_t)r * p.Kb; };
        oa0 = rowoff(m0 + lrow, p.M); oa1 = rowoff(m0 + lrow + 64, p.M);
        oa2 = rowoff(m0 + lrow + 128, p.M); oa3 = rowoff(m0 + lrow + 192, p.M);
        ob0 = rowoff(n0 + lrow, p.N); ob1 = rowoff(n0 + lrow + 64, p.N);
        ob2 = rowoff(n0 + lrow + 128, p.N); ob3 = rowoff(n0 + lrow + 192, p.N);
    }
    const int s0 = swz2(lrow, lslot), s1 = swz2(lrow + 64, lslot), s2 = swz2(lrow + 128, lslot), s3 = swz2(lrow + 192, lslot);

    typename Acc<DT>::type acc[TM][2];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

    const int nk = (int)(p.Kb / BK2);
    uint4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;
    ra1 = ra2 = ra3 = make_uint4(0, 0, 0, 0);
    // GENA: the raw fp32 values of this thread's (row, 16-element slot) pairs, and the quantiser
    [[maybe_unused]] float4 xg[GENA ? 2 : 1][4];
    [[maybe_unused]] const float* xr0 = nullptr;
    [[maybe_unused]] const float* xr1 = nullptr;
    [[maybe_unused]] float g_s = 1.0f, g_inv = 1.0f, g_lo = 0.0f, g_hi = 0.0f;
    if constexpr (GENA) {
        const float* xb = p.gen_x + (int64_t)g * p.gen_sg + lslot * 16;
        int r0 = min(m0 + lrow, p.M - 1), r1 = min(m0 + lrow + 64, p.M - 1);
        if constexpr (ROWMAP) {
            if (p.a_rows) {
                const int i0 = r0 / p.row_period, i1 = r1 / p.row_period;
                r0 = p.a_rows[r0 - i0 * p.row_period] + i0 * p.row_period;
                r1 = p.a_rows[r1 - i1 * p.row_period] + i1 * p.row_period;
            }
        }
        xr0 = xb + (int64_t)r0 * p.gen_ldx;
        xr1 = xb + (int64_t)r1 * p.gen_ldx;
        g_s = p.gen_scale[gh * p.gen_sn];
        const float z = rintf(p.gen_zp[gh * p.gen_sn]);
        g_inv = __builtin_amdgcn_rcpf(g_s);
        g_lo = -z; g_hi = p.gen_qmax - z;
    }
    auto gen_load = [&](int kt) {
        if constexpr (GENA) {
            const bool kv = kt * BK2 + lslot * 16 < p.gen_K;                // (gen_K % 16 == 0: a slot is all valid or all padding)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                xg[0][j] = kv ? *reinterpret_cast<const float4*>(xr0 + kt * BK2 + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
                if (TM >= 2) xg[1][j] = kv ? *reinterpret_cast<const float4*>(xr1 + kt * BK2 + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    auto gen_pack = [&](const float4 (&x4)[4]) {
#pragma clang fp contract(off)
        float xv[16], kq[16], dm = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) { xv[4 * j] = x4[j].x; xv[4 * j + 1] = x4[j].y; xv[4 * j + 2] = x4[j].z; xv[4 * j + 3] = x4[j].w; }
#pragma unroll
        for (int e = 0; e < 16; ++e) { const float t = xv[e] * g_inv; kq[e] = rintf(t); dm = fmaxf(dm, fabsf(t - kq[e])); }
        if (__builtin_expect(dm > 0.4999f, 0)) {                             // tie zone (operand.hip k_pack_kfast): the IEEE quotient decides
#pragma unroll
            for (int e = 0; e < 16; ++e) kq[e] = rintf(xv[e] / g_s);
        }
        uint4 o;
        unsigned* ow = reinterpret_cast<unsigned*>(&o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned pk = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) pk = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_amdgcn_fmed3f(kq[4 * j + e], g_lo, g_hi) + 128.0f, e, pk);
            ow[j] = pk ^ 0x80808080u;
        }
        return o;
    };
#define GLOAD(KT)                                                                              \
    do {                                                                                       \
        const int64_t ko = (int64_t)(KT) * BK2;                                                \
        if constexpr (GENA) gen_load(KT);                                                      \
        else {                                                                                 \
        ra0 = *reinterpret_cast<const uint4*>(Ab + oa0 + ko);                                  \
        if (TM >= 2) ra1 = *reinterpret_cast<const uint4*>(Ab + oa1 + ko);                     \
        if (TM >= 4) { ra2 = *reinterpret_cast<const uint4*>(Ab + oa2 + ko);                   \
                       ra3 = *reinterpret_cast<const uint4*>(Ab + oa3 + ko); }                 \
        }                                                                                      \
        rb0 = *reinterpret_cast<const uint4*>(Bb + ob0 + ko);                                  \
        rb1 = *reinterpret_cast<const uint4*>(Bb + ob1 + ko);                                  \
        rb2 = *reinterpret_cast<const uint4*>(Bb + ob2 + ko);                                  \
        rb3 = *reinterpret_cast<const uint4*>(Bb + ob3 + ko);                                  \
    } while (0)
#define SSTORE()                                                                               \
    do {                                                                                       \
        if constexpr (GENA) { ra0 = gen_pack(xg[0]); if (TM >= 2) ra1 = gen_pack(xg[1]); }     \
        *reinterpret_cast<uint4*>(As + s0) = ra0;                                              \
        if (TM >= 2) *reinterpret_cast<uint4*>(As + s1) = ra1;                                 \
        if (TM >= 4) { *reinterpret_cast<uint4*>(As + s2) = ra2;                               \
                       *reinterpret_cast<uint4*>(As + s3) = ra3; }                             \
        *reinterpret_cast<uint4*>(Bs + s0) = rb0; *reinterpret_cast<uint4*>(Bs + s1) = rb1;    \
        *reinterpret_cast<uint4*>(Bs + s2) = rb2; *reinterpret_cast<uint4*>(Bs + s3) = rb3;    \
    } while (0)
    GLOAD(0);
    SSTORE();
    __syncthreads();

    const int frow = lane & 31, fkg = lane >> 5;
    const int arow = wr * (BM2 / 2) + frow, brow = wc * 64 + frow;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) GLOAD(kt + 1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            uint4 af[TM], bf[2];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const uint4*>(As + swz2(arow + i * 32, ks * 2 + fkg));
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const uint4*>(Bs + swz2(brow + j * 32, ks * 2 + fkg));
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mma<DT>(af[i], bf[j], acc[i][j]);
        }
        if (kt + 1 < nk) {
            __syncthreads();
            SSTORE();
            __syncthreads();
        }
    }
#undef GLOAD
#undef SSTORE

    const bool edge = (m0 + BM2 > p.M) || (n0 + BN2 > p.N);
    const bool rows = p.row_scale != nullptr;
    const bool lds_ref = !STORE && p.ldr == 1 && p.ref_div >= 32 && (BN2 % p.ref_div) == 0;
    if (lds_ref) {
        __syncthreads();                                   // every wave is done with the operand tiles: reuse As as staging
        float* stage = reinterpret_cast<float*>(smem);
        if (edge) {
            if (rows) epilogue_lds<DT, TM, true, true>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red, stage);
            else epilogue_lds<DT, TM, true, false>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red, stage);
        } else {
            if (rows) epilogue_lds<DT, TM, false, true>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red, stage);
            else epilogue_lds<DT, TM, false, false>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red, stage);
        }
    } else if (edge) {
        if (rows) epilogue2<DT, TM, STORE, true, true, ADD, ROWMAP>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red);
        else epilogue2<DT, TM, STORE, true, false, ADD, ROWMAP>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red);
    } else {
        if (rows) epilogue2<DT, TM, STORE, false, true, ADD, ROWMAP>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red);
        else epilogue2<DT, TM, STORE, false, false, ADD, ROWMAP>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red);
    }
    if (!STORE && p.partial) {
        __syncthreads();
        float v = 0.0f;
        const int col = n0 + tid;                                      // tid < 256: column tid of the tile
        if (tid < 256) v = red[tid] + red[256 + tid];                  // wr = 0 plus wr = 1 (index = wc*64 + j*32 + lane)
        if (p.reduce_cols) {
            if (tid < 256) colv[tid] = v;
            __syncthreads();
            if (tid < 64) {
                float t2 = (colv[tid] + colv[tid + 64]) + (colv[tid + 128] + colv[tid + 192]);
#pragma unroll
                for (int sft = 32; sft > 0; sft >>= 1) t2 += __shfl_xor(t2, sft);
                if (tid == 0) p.partial[(((int64_t)g) * p.MT + mt) * p.Npad + nt] = t2;
            }
        } else if (tid < 256) {
            if (p.ref_div > 1) {
                if (col < p.N)
                    p.partial[((((int64_t)g) * p.MT + mt) * p.Npad + col / p.ref_div) * p.ref_div + col % p.ref_div] = v;
            } else if (col < p.Npad) {
                p.partial[(((int64_t)g) * p.MT + mt) * p.Npad + col] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ LDS-DMA pipelined variant
// Same tile and epilogues as k_gemm_cand, but the operand tiles go global -> LDS directly (global_load_lds_dwordx4, no
// VGPR round trip, no ds_write pass) into a ring of NS = 3 stages, with counted vmcnt and raw s_barrier so that two
// K-steps of loads stay in flight across the barrier (cdna guide section 5: "glds span barrier").  The LDS destination of
// an LDS-DMA is lane-linear (wave base + lane*16), so the bank swizzle is applied to the per-lane GLOBAL source address
// (rule 21): lane l of a request covering 8 rows fetches logical slot (l & 7) ^ ((row >> 1) & 7) of row (l >> 3).
typedef const void __attribute__((address_space(1)))* gas_ptr;
typedef void __attribute__((address_space(3)))* las_ptr;

// One K-step of the LDS-DMA pipeline.  `cur` (stage being read) and `nxt` (ring slot being refilled) are __restrict__ so
// that, after inlining, the DMA stores and the fragment reads carry disjoint alias scopes: without them the waitcnt
// insertion pass must assume the ds_reads alias the in-flight LDS-DMA and drains vmcnt(0) every step.
template <int DT, int TM, int NA>
__device__ __forceinline__ void glds_step(const uint8_t* __restrict__ cur, uint8_t* __restrict__ nxt, bool do_issue,
                                          const uint8_t* Ab, const uint8_t* Bb, const int64_t (&oa)[NA], const int64_t (&ob)[4],
                                          const int (&la)[NA], const int (&lb)[4], int64_t ko, int arow, int brow, int fkg,
                                          typename Acc<DT>::type (&acc)[TM][2]) {
    constexpr int BM2 = 64 * TM;
    if (do_issue) {
#pragma unroll
        for (int i = 0; i < NA; ++i)
            __builtin_amdgcn_global_load_lds((gas_ptr)(Ab + oa[i] + ko), (las_ptr)(nxt + la[i]), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((gas_ptr)(Bb + ob[i] + ko), (las_ptr)(nxt + lb[i]), 16, 0, 0);
    }
    const uint8_t* As = cur;
    const uint8_t* Bs = cur + BM2 * BK2;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        uint4 af[TM], bf[2];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const uint4*>(As + swz2(arow + i * 32, ks * 2 + fkg));
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const uint4*>(Bs + swz2(brow + j * 32, ks * 2 + fkg));
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) mma<DT>(af[i], bf[j], acc[i][j]);
    }
}

template <int DT, int TM>
__global__ __launch_bounds__(512, 2) void k_gemm_cand_glds(GemmArgs p) {
    constexpr int BM2 = 64 * TM;
    constexpr int STAGE = (BM2 + BN2) * BK2;
    constexpr int NS = 3;
    constexpr int NA = BM2 / 64;                   // 8-row requests per wave for the A tile (BM2/8 requests over 8 waves)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* red = reinterpret_cast<float*>(smem + NS * STAGE);
    float* colv = red + 512;

    const unsigned nwg = gridDim.x, bid = blockIdx.x;
    const unsigned q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    const unsigned lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    TL_STAMP(0);
    unsigned t = lid;
    int nt, mt, g;
    if (p.order == 2) { mt = t % p.MT; t /= p.MT; nt = t % p.NT; g = t / p.NT; }
    else { nt = t % p.NT; t /= p.NT; mt = t % p.MT; g = t / p.MT; }
    const int gh = g % p.gmod;
    const int m0 = mt * BM2, n0 = nt * BN2;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = w >> 2, wc = w & 3;
    const int lr = lane >> 3, lslot = lane & 7;
    // per-lane global sources: A requests rbA = w*NA + i (i < NA), B requests rbB = w*4 + i (i < 4); 8 rows per request
    const uint8_t* Ab = p.A + g * p.sAg;
    const uint8_t* Bb = p.B + g * p.sBg;
    int64_t oa[NA], ob[4];
    int la[NA], lb[4];                              // wave-uniform LDS byte offsets of the requests inside a stage
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int rl = (w * NA + i) * 8 + lr;       // row inside the tile
        int r = m0 + rl; r = r < p.M ? r : p.M - 1;
        oa[i] = (int64_t)r * p.Kb + ((lslot ^ ((rl >> 1) & 7)) << 4);
        la[i] = (w * NA + i) * 1024;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rl = (w * 4 + i) * 8 + lr;
        int r = n0 + rl; r = r < p.N ? r : p.N - 1;
        ob[i] = (int64_t)r * p.Kb + ((lslot ^ ((rl >> 1) & 7)) << 4);
        lb[i] = BM2 * BK2 + (w * 4 + i) * 1024;
    }
    auto issue = [&](int kt) {
        uint8_t* st = smem + (kt % NS) * STAGE;
        const int64_t ko = (int64_t)kt * BK2;
#pragma unroll
        for (int i = 0; i < NA; ++i)
            __builtin_amdgcn_global_load_lds((gas_ptr)(Ab + oa[i] + ko), (las_ptr)(st + la[i]), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((gas_ptr)(Bb + ob[i] + ko), (las_ptr)(st + lb[i]), 16, 0, 0);
    };

    typename Acc<DT>::type acc[TM][2];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

    const int nk = (int)(p.Kb / BK2);
    issue(0);
    if (nk > 1) issue(1);
    TL_STAMP(1);
    const int frow = lane & 31, fkg = lane >> 5;
    const int arow = wr * (BM2 / 2) + frow, brow = wc * 64 + frow;
    for (int kt = 0; kt < nk; ++kt) {
        // stage kt has landed once at most one later stage (NA + 4 requests of this wave) is still outstanding
        if (kt + 1 < nk) {
            if (NA == 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();               // everyone's part of stage kt landed; everyone finished stage kt-1
        asm volatile("" ::: "memory");
        if (kt == 0) TL_STAMP(2);
        glds_step<DT, TM, NA>(smem + (kt % NS) * STAGE, smem + ((kt + 2) % NS) * STAGE, kt + 2 < nk, Ab, Bb, oa, ob, la, lb,
                              (int64_t)(kt + 2) * BK2, arow, brow, fkg, acc);
    }

    const bool edge = (m0 + BM2 > p.M) || (n0 + BN2 > p.N);
    const bool rows = p.row_scale != nullptr;
    const bool lds_ref = p.ldr == 1 && p.ref_div >= 32 && (BN2 % p.ref_div) == 0;
    TL_STAMP(3);
    __syncthreads();
    TL_STAMP(4);
    if (lds_ref) {
        float* stage = reinterpret_cast<float*>(smem);
        if (edge) {
            if (rows) epilogue_lds<DT, TM, true, true>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red, stage);
            else epilogue_lds<DT, TM, true, false>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red, stage);
        } else {
            if (rows) epilogue_lds<DT, TM, false, true>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red, stage);
            else epilogue_lds<DT, TM, false, false>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red, stage);
        }
    } else if (edge) {
        if (rows) epilogue2<DT, TM, false, true, true>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red);
        else epilogue2<DT, TM, false, true, false>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red);
    } else {
        if (rows) epilogue2<DT, TM, false, false, true>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red);
        else epilogue2<DT, TM, false, false, false>(p, acc, g, gh, m0, n0, wr, wc, frow, fkg, red);
    }
    TL_STAMP(5);
    if (p.partial) {
        __syncthreads();
        TL_STAMP(6);
        float v = 0.0f;
        const int col = n0 + tid;
        if (tid < 256) v = red[tid] + red[256 + tid];
        if (p.reduce_cols) {
            if (tid < 256) colv[tid] = v;
            __syncthreads();
            if (tid < 64) {
                float t2 = (colv[tid] + colv[tid + 64]) + (colv[tid + 128] + colv[tid + 192]);
#pragma unroll
                for (int sft = 32; sft > 0; sft >>= 1) t2 += __shfl_xor(t2, sft);
                if (tid == 0) p.partial[(((int64_t)g) * p.MT + mt) * p.Npad + nt] = t2;
            }
        } else if (tid < 256) {
            if (p.ref_div > 1) {
                if (col < p.N)
                    p.partial[((((int64_t)g) * p.MT + mt) * p.Npad + col / p.ref_div) * p.ref_div + col % p.ref_div] = v;
            } else if (col < p.Npad) {
                p.partial[(((int64_t)g) * p.MT + mt) * p.Npad + col] = v;
            }
        }
    }
    TL_STAMP(7);
}

