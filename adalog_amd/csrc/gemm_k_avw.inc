// Part of gemm_score.hip (one translation unit, included inside its anonymous namespace): the softmax.v WEIGHT search with its candidate
// operand generated in registers (reference quant_layers/matmul.py:173-201: the search over the uniform quantiser of v).
//
// k_gemm_grpk8t gives each of its seven consumer waves one 32-row block of the attention rows and streams the packed fp8 candidate
// columns ([G][64 x 128][208], 310 MB per launch for deit_small) past them: every wave needs every candidate fragment, so the
// fragments have to exist in memory.  Here the WAVE OWNS THE CANDIDATES: wave w of a workgroup holds the (scale, zero point) of
// candidates 32 w .. 32 w + 31 -- one per lane column -- and for a head-dim column d of v builds the MFMA B fragment of the block
// (d, 32 w ..) itself from the fp32 row v^T[d][0 .. K): 8 values per lane and MFMA, the same 8 for the 32 lanes of a half wave.  It
// multiplies the fragment against ALL row blocks of the fixed operand -- the post-softmax AdaLog image of the group, resident in LDS
// -- so no fragment is generated twice and no candidate ever reaches memory.
//
// The scores are those of pack + k_gemm_grpk8t<NJ, 13> bit for bit, by construction:
//   * operand: per element  t = x * (1 / s), rne, the IEEE quotient where some |t - rne t| of the lane's 8 values is inside the tie
//     zone, med3 against (-z, qmax - z)  -- uni_codes / uni_clamp of operand.hip; the integer (|.| <= 15) is exact in bf16, as the
//     fp8 byte the packer stores and fp8x16_bf16 converts back is;
//   * product: MFMA i of a block multiplies K = 32 (i >> 1) + 16 fkg + 8 (i & 1) + 0..7, i = 0..12 in this order, into one fp32
//     accumulator tile per row block -- k_gemm_grpk8t's instruction, operands and order (K 208..215 of MFMA 12, fkg 1: zero rows);
//   * epilogue: d = fma(acc, -(sa sa_mul sb), ref), then x += d0^2, y += d1^2, x += d2^2, y += d3^2 per row quad into one fp32 pair
//     per (row block, lane) that runs over the head-dim columns of the item in order; x + y, the lane pair, the row blocks in fp64
//     in order, the items of a workgroup in order: the same items (grp_chunks) on the same grid, so [workgroup][head][256] holds
//     the same sums.
// Items are k_gemm_grpk8t's (group, chunk of CB column blocks); the workgroup has NJ waves (one per 32 candidates), and with the
// 79 KB image of a 197-row group two workgroups share a CU: two waves per SIMD, one generating while the other multiplies.
//   LDS: [MI + 1 rows][25 slots of 16 bytes] + 64 bytes: K < 200 of the packed bf16 rows; rows from M on and the tail all zero.
//   M > 192: MI = M, rows past M read row M; otherwise MI = M rounded up to 32, so every row block is whole and 12 800 bytes from
//   the last (the upper half wave of MFMA 12 reads the 32 bytes behind its row against a zero B fragment).  25 slots: an odd
//   stride, so the 16 rows of a ds_read_b128 lane group fall on 16 different slots of the 256-byte bank row.
//   Behind the image: the fp32 REFERENCE COLUMN of the head-dim column in work, [224] floats, zero from row M on (such rows meet a
//   zero accumulator and must add nothing): the quad of rows a lane's epilogue needs is one ds_read_b128.  The column depends on
//   (row, d) only: staged once per workgroup, every wave and both half waves read it (the 32 lanes of a half wave the same address:
//   a broadcast).  Two buffers, alternating over d, where two workgroups of that size still share a CU (M <= 199); one buffer
//   and a second barrier per column otherwise.
constexpr int AVW_REF_BYTES = 224 * 4;
__host__ __device__ constexpr int avw_img_rows(int M) { return M > 192 ? M : (M + 31) & ~31; }
__host__ __device__ constexpr int avw_img_bytes(int M) { return (avw_img_rows(M) + 1) * 400 + 64; }
__host__ __device__ constexpr bool avw_ref_two(int M) { return 2 * (avw_img_bytes(M) + 2 * AVW_REF_BYTES) <= 160 * 1024; }
__host__ __device__ constexpr int avw_lds_bytes(int M) { return avw_img_bytes(M) + (avw_ref_two(M) ? 2 : 1) * AVW_REF_BYTES; }
struct AvwCand { float s, inv, lo, hi; };
__device__ __forceinline__ uint4 avw_gen8(const v4u& xa, const v4u& xb, const AvwCand& c) {
#pragma clang fp contract(off)
    const float x[8] = {__uint_as_float(xa.x), __uint_as_float(xa.y), __uint_as_float(xa.z), __uint_as_float(xa.w),
                        __uint_as_float(xb.x), __uint_as_float(xb.y), __uint_as_float(xb.z), __uint_as_float(xb.w)};
    float k[8], dm = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float t = x[e] * c.inv;
        k[e] = rintf(t);
        dm = fmaxf(dm, fabsf(t - k[e]));
    }
    if (__builtin_expect(dm > 0.4999f, 0)) {
#pragma unroll
        for (int e = 0; e < 8; ++e) k[e] = rintf(x[e] / c.s);
    }
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t v0 = __float_as_uint(__builtin_amdgcn_fmed3f(k[2 * e], c.lo, c.hi));
        const uint32_t v1 = __float_as_uint(__builtin_amdgcn_fmed3f(k[2 * e + 1], c.lo, c.hi));
        w[e] = __builtin_amdgcn_perm(v1, v0, 0x07060302u);     // the top halves: small integers are exact in bf16
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int NJ, bool R7>
__global__ __launch_bounds__(NJ * 64, 2) void k_gemm_avw_gen(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int NKS = 13, ASL = 25, ARB = ASL * 16, NT = NJ * 64, LA = 2;
    constexpr int IU = 10;                                     // image slots a lane has in flight at once
    constexpr int RPT = (224 + NT - 1) / NT;                   // reference rows a lane stages
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fkg = lane >> 5;
    const int M = p.M, KbA = (int)p.KbA;
    const int nrb = R7 ? 7 : (M + 31) >> 5;
    const int NB = p.N >> 5;
    const int CB = p.slab_R, NCH = p.slab_U;
    const int items = p.G * NCH;
    const int ci = w * 32 + frow;
    double* wacc = p.wg_acc + (int64_t)blockIdx.x * p.gmod * 256;
    for (int i = tid; i < p.gmod * 256; i += NT) wacc[i] = 0.0;

    // LDS byte offset of this lane's fragment of row block rb for MFMA 0 (MFMA i: + 64 (i >> 1) + 16 (i & 1)); with 7 row blocks
    // (M > 192) the first six are whole and 12 800 bytes apart, which is an instruction's immediate; with fewer all are whole
    const int base0 = frow * ARB + fkg * 32, base6 = min(192 + frow, M) * ARB + fkg * 32;
    auto aoff = [&](int rb) { return rb < 6 ? base0 + rb * 32 * ARB : base6; };
    const int xvoff = fkg * 64;                                // MFMA i reads K = 32 (i >> 1) + 16 fkg + 8 (i & 1) + 0..7 of a row of v^T
    // the image slots of this lane: tid, tid + NT, .. as (row, slot of the row), stepped without a division
    const int ir0 = tid / ASL, is0 = tid - ir0 * ASL;
    const int islots = (avw_img_rows(M) + 1) * ASL + 4;
    const int nsl = min(ASL, KbA >> 4);                        // slots a packed row has (shorter rows: zeros behind them)
    // the reference column(s) behind the image; a lane's row quad q of row block rb is rows 32 rb + 8 q + 4 fkg + 0..3
    const int refo = avw_img_bytes(M) + fkg * 16;
    const bool two = avw_ref_two(M);

    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int g = item / NCH, c = item - g * NCH, gh = g % p.gmod;
        const int blk0 = c * CB, nblk = min(CB, NB - blk0);
        const int d0 = blk0 / NJ, nd = nblk / NJ;
        const float* refg = p.ref + (int64_t)g * p.sRg;
        // rows 0 .. 223 of the reference column d (zero from M on): this lane's, from memory / into buffer b
        auto ref_fetch = [&](int d, float (&r)[RPT]) {
            const float* rp = refg + (int64_t)d * p.ref_cs;
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                const int t = tid + u * NT;
                r[u] = t < M ? rp[t] : 0.0f;
            }
        };
        auto ref_put = [&](int b, const float (&r)[RPT]) {
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                const int t = tid + u * NT;
                if (t < 224) *reinterpret_cast<float*>(lds + avw_img_bytes(M) + b * AVW_REF_BYTES + t * 4) = r[u];
            }
        };
        __syncthreads();                                       // the previous item's fragment and reference reads are done (and wacc is zeroed)
        {
            // IU loads in flight per lane and round trip; a slot outside the packed rows reads slot 0 and is stored as zero
            const uint8_t* ag = p.A + (int64_t)g * p.sAg;
            float r0[RPT];
            ref_fetch(d0, r0);
            int r = ir0, s = is0;
            for (int idx = tid; idx < islots; idx += IU * NT) {
                uint4 v[IU];
#pragma unroll
                for (int u = 0; u < IU; ++u) {
                    const bool in = r < M && s < nsl;
                    v[u] = *reinterpret_cast<const uint4*>(ag + (in ? r * KbA + s * 16 : 0));
                    if (!in) v[u] = make_uint4(0, 0, 0, 0);
                    r += NT / ASL; s += NT % ASL;
                    if (s >= ASL) { s -= ASL; ++r; }
                }
#pragma unroll
                for (int u = 0; u < IU; ++u)
                    if (idx + u * NT < islots) *reinterpret_cast<uint4*>(lds + (idx + u * NT) * 16) = v[u];   // slot idx = 25 row + slot
            }
            ref_put(0, r0);
        }
        __syncthreads();

        AvwCand cand;
        {
            const int64_t pi = ci * p.sb_c + gh * p.sb_g;
            const float z = rintf(p.gen_zp[pi]);
            cand.s = p.sb[pi]; cand.inv = __builtin_amdgcn_rcpf(cand.s); cand.lo = -z; cand.hi = p.gen_qmax - z;
        }
        const float nal = -(p.sa[ci * p.sa_c + gh * p.sa_g] * p.sa_mul * p.sb[ci * p.sb_c + gh * p.sb_g]);
        const int64_t xbytes = ((int64_t)(p.N / (NJ * 32)) * p.gen_ldx) * 4;      // one group of v^T: past it a load reads zeros
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(p.gen_x + (int64_t)g * p.gen_sg), 0,
                                                                            (int)min(xbytes, (int64_t)0x7ffffffe), 0x00020000);
        // 16-byte loads at the 4-byte alignment of a row of K floats.  MFMA i reads elements up to 32 (i >> 1) + 16 fkg + 8 (i & 1) + 7 <= 215
        // of row d: past K they are the next row's values (zeros past the group), and candidates are generated from them all the same.
        // That is harmless on two conditions: x is finite, and the fixed operand is zero from K on (the packer's padding up to element
        // 207); the upper half wave of MFMA 12, whose x would be elements 208 .. 215, gets a zero fragment instead.  So every such
        // product is 0 x finite.
        auto load_x = [&](int d, int i, v4u& xa, v4u& xb) {
            // lane part (the K half) in the VGPR, the row in the SGPR, the MFMA's K offset an immediate
            const int so = d * (int)p.gen_ldx * 4;
            xa = __builtin_amdgcn_raw_buffer_load_b128(rx, xvoff + (32 * (i >> 1) + 8 * (i & 1)) * 4, so, 0);
            xb = __builtin_amdgcn_raw_buffer_load_b128(rx, xvoff + (32 * (i >> 1) + 8 * (i & 1)) * 4 + 16, so, 0);
        };
        auto load_a = [&](int i, uint4 (&af)[7]) {
#pragma unroll
            for (int rb = 0; rb < 7; ++rb)
                if (R7 || rb < nrb) af[rb] = *reinterpret_cast<const uint4*>(lds + aoff(rb) + (i >> 1) * 64 + (i & 1) * 16);
        };
        auto load_ref = [&](int b, int rb, float (&r)[16]) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 t = *reinterpret_cast<const float4*>(lds + refo + b * AVW_REF_BYTES + (rb * 32 + 8 * q) * 4);
                r[4 * q + 0] = t.x; r[4 * q + 1] = t.y; r[4 * q + 2] = t.z; r[4 * q + 3] = t.w;
            }
        };

        v2f csr[7];
#pragma unroll
        for (int rb = 0; rb < 7; ++rb) csr[rb] = (v2f){0.0f, 0.0f};

        // x of the first LA MFMAs of the coming block, the B fragment and the row fragments of its MFMA 0
        v4u xq[NKS + LA][2];
#pragma unroll
        for (int i = 0; i < LA; ++i) load_x(d0, i, xq[i][0], xq[i][1]);
        for (int dd = 0; dd < nd; ++dd) {
            const int d = d0 + dd, dn = d0 + min(dd + 1, nd - 1);
            // the reference column of the next d travels during this block's MFMAs (two buffers)
            float rnx[RPT];
            if (two && dd + 1 < nd) ref_fetch(d + 1, rnx);
            v16f acc[7];
#pragma unroll
            for (int rb = 0; rb < 7; ++rb)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[rb][e] = 0.0f;
            uint4 bq = avw_gen8(xq[0][0], xq[0][1], cand);
#pragma unroll
            for (int i = 0; i < NKS; ++i) {
                uint4 af[7];
                load_a(i, af);
                if (i + LA < NKS) load_x(d, i + LA, xq[i + LA][0], xq[i + LA][1]);
                else load_x(dn, i + LA - NKS, xq[i + LA][0], xq[i + LA][1]);
                uint4 bn = bq;
                if (i + 1 < NKS) bn = avw_gen8(xq[i + 1][0], xq[i + 1][1], cand);
                // MFMA 12 has no K for the upper half wave (K 208..215): zeros against the (finite) bytes behind the row
                if (i + 1 == 12 && fkg) bn = make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int rb = 0; rb < 7; ++rb)
                    if (R7 || rb < nrb) mma<1>(af[rb], bq, acc[rb]);
                bq = bn;
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int i = 0; i < LA; ++i) { xq[i][0] = xq[NKS + i][0]; xq[i][1] = xq[NKS + i][1]; }
            // the reference column of this block is buffer dd & 1, staged one block ago; the barrier hands the other buffer (read
            // by the last block's epilogue) over to the next column.  One buffer: wait for the last epilogue, stage, wait again.
            int rbuf = 0;
            if (two) {
                __syncthreads();
                if (dd + 1 < nd) ref_put((dd + 1) & 1, rnx);
                rbuf = dd & 1;
            } else if (dd > 0) {
                __syncthreads();
                ref_fetch(d, rnx);
                ref_put(0, rnx);
                __syncthreads();
            }
            // epilogue of the seven 32 x 32 tiles
#pragma unroll
            for (int rb = 0; rb < 7; ++rb) {
                if (R7 || rb < nrb) {
                    float rc[16];
                    load_ref(rbuf, rb, rc);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float e0 = __builtin_fmaf(acc[rb][q * 4 + 0], nal, rc[q * 4 + 0]);
                        const float e1 = __builtin_fmaf(acc[rb][q * 4 + 1], nal, rc[q * 4 + 1]);
                        const float e2 = __builtin_fmaf(acc[rb][q * 4 + 2], nal, rc[q * 4 + 2]);
                        const float e3 = __builtin_fmaf(acc[rb][q * 4 + 3], nal, rc[q * 4 + 3]);
                        csr[rb].x = __builtin_fmaf(e0, e0, csr[rb].x); csr[rb].y = __builtin_fmaf(e1, e1, csr[rb].y);
                        csr[rb].x = __builtin_fmaf(e2, e2, csr[rb].x); csr[rb].y = __builtin_fmaf(e3, e3, csr[rb].y);
                    }
                }
            }
        }
        double v = 0.0;
#pragma unroll
        for (int rb = 0; rb < 7; ++rb) {
            if (R7 || rb < nrb) {
                float cs = csr[rb].x + csr[rb].y;
                cs += __shfl_xor(cs, 32);
                v += (double)cs;
            }
        }
        if (fkg == 0) wacc[gh * 256 + ci] += v;
    }
#endif
}
