// The GPTQ sweep kernel (layout and specification: gptq.hip), included twice by gptq.hip with
//   SWEEP_KERNEL  the kernel's name
//   SWEEP_PERM    0: columns in natural order;  1: step j works on column perm[j] (act-order) -- the load of the running row gathers
//                 through perm and the per-block store scatters through it, nothing in between changes.
template <int NI_MAX, int G, int RPW>
__global__ __launch_bounds__(256) void SWEEP_KERNEL(const float* __restrict__ w, int64_t R, int K, int64_t ldw,
                                                    const float* __restrict__ scale, const float* __restrict__ zp, int per_row,
                                                    float qmax, const double* __restrict__ U, int64_t ldu,
#if SWEEP_PERM
                                                    const int32_t* __restrict__ perm,
#endif
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
#if SWEEP_PERM
            run[r][i] = col < K ? (double)w[rows[r] * ldw + perm[col]] : 0.0;   // step ``col`` works on column perm[col]
#else
            run[r][i] = col < K ? (double)w[rows[r] * ldw + col] : 0.0;
#endif
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
#if SWEEP_PERM
        const int dst = col < K ? perm[col] : 0;                     // ... and leaves its results there: natural order
#pragma unroll
        for (int r = 0; r < RPW; ++r)
            if (col < K && row0 + r < R) {
                what[rows[r] * (int64_t)K + dst] = qv[r];
                if (codes) codes[rows[r] * (int64_t)K + dst] = (uint8_t)(int)cv[r];
            }
#else
#pragma unroll
        for (int r = 0; r < RPW; ++r)
            if (col < K && row0 + r < R) {
                what[rows[r] * (int64_t)K + col] = qv[r];
                if (codes) codes[rows[r] * (int64_t)K + col] = (uint8_t)(int)cv[r];
            }
#endif
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
