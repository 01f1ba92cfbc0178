// Hessian bit cost of one layer's weight at several widths in ONE launch (utils/bitplan.py; no counterpart in the reference).
//
// Specification (include/adalog_hip.h), for width i and row r of w [R][K], H fp64 [K][K] symmetric:
//   bits[i] == 0:  d_j = double(w[r][j])                                                         (the signal row: w H w^T)
//   else:          c_j = uni_bin(w[r][j], s, rne(z), 2^b - 1)     fp32, the function k_gptq_sweep / pack_codes use (common.h)
//                  q_j = (c_j - rne(z)) * s                        fp32, as unpack_codes(F32) computes it
//                  d_j = double(w[r][j]) - double(q_j)
//   cost[i][r] = sum_j sum_k d_j H[j][k] d_k        products and sums in fp64
// The order of the sums is this kernel's own and is fixed: two calls return the same bits (no floating-point atomics).
//
// Layout.  A workgroup (4 waves) owns a tile of 16 rows, ALL widths, and a run of 64-column chunks of H.  For a chunk it forms
// E = D . H[:, chunk] (16 x 64 per width) on v_mfma_f64_16x16x4_f64 and folds the row dot sum_c E[r][c] * D[r][c] in the epilogue, so
// neither D nor E ever reaches global memory:
//   - H is staged through LDS in tiles of 32 rows x 64 columns (the next tile's global loads are in flight during the MFMAs) and one
//     staged tile serves every width of the workgroup; the 16 x 32 tile of w is staged beside it.
//   - A wave owns widths and 16-column tiles of the chunk: widths {wave, wave + 4} x 4 column tiles for 3 .. 8 widths, one width x 2
//     column tiles for 2 widths, 1 column tile for a single width.  The A fragment (lane l: row l & 15, k = l >> 4) is produced in
//     registers from the staged w for each width of the wave; a B fragment (lane l: k = l >> 4, column l & 15) is read once per
//     K-step and feeds the MFMAs of all the wave's widths.
//   - C/D of the f64 form: lane l, register i holds row (l >> 4) + 4 i, column l & 15 -- NOT the f32 forms' map.  The epilogue
//     recomputes d of exactly those elements from w (global, 16 x 64 elements per chunk) and multiplies.
// The chunks of a row tile are split over `nsplit` workgroups when there are few row tiles (fixed rule, bc_geo below); a workgroup
// then leaves nw x 16 fp64 partials in the workspace, draws the row tile's ticket, and the last arriver adds the partials in split
// order (agent-scope stores and loads around the ticket, as select.hip's k_sel_hist_pick orders them).
#include "common.h"
#include "fpcs_tail.h"

#pragma clang fp contract(off)

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int MAXW = 8;            // widths per call
constexpr int RT = 16;             // rows per tile (the MFMA's M)
constexpr int CN = 64;             // columns of H per chunk
constexpr int KB = 32;             // rows of H per staged tile
constexpr int HLD = CN + 16;       // LDS row stride of the H tile in doubles: rows 640 bytes apart, so the four k-rows a B fragment
                                   // touches start 128 bytes apart modulo the 256 bytes of the banks
constexpr int WLD = KB + 1;        // ... of the w tile in floats
constexpr int TARGET_WGS = 512;    // the chunks of a row tile are split until about this many workgroups exist

struct Widths {
    int bits[MAXW];
};

struct Geo {
    int64_t tiles;                 // row tiles
    int nchunks, cpw, nsplit;      // 64-column chunks, chunks per workgroup, workgroups per row tile
};

inline Geo bc_geo(int64_t R, int64_t K) {
    Geo g;
    g.tiles = (R + RT - 1) / RT;
    g.nchunks = (int)((K + CN - 1) / CN);
    int64_t want = (TARGET_WGS + g.tiles - 1) / g.tiles;
    if (want > g.nchunks) want = g.nchunks;
    if (want < 1) want = 1;
    g.cpw = (int)((g.nchunks + want - 1) / want);
    g.nsplit = (g.nchunks + g.cpw - 1) / g.cpw;
    return g;
}

inline int64_t part_doubles(const Geo& g, int nw) { return g.nsplit > 1 ? g.tiles * g.nsplit * nw * RT : 0; }

// d of the specification for one element
__device__ __forceinline__ double bc_d(float w, float s, float z, float qmax, bool signal) {
    if (signal) return (double)w;
    const float c = uni_bin(w, s, z, qmax);
    const float q = (c - z) * s;
    return (double)w - (double)q;
}

template <int WPW>
__global__ __launch_bounds__(256) void k_bit_cost(const float* __restrict__ w, int64_t R, int K, int64_t ldw,
                                                  const float* __restrict__ scale, const float* __restrict__ zp, int per_row,
                                                  Widths wd, int nw, const double* __restrict__ H, int64_t ldh,
                                                  double* __restrict__ cost, double* part, unsigned int* tickets, Geo geo) {
    __shared__ double Ht[KB * HLD];
    __shared__ float Wt[RT * WLD];
    __shared__ float ps[MAXW][RT], pz[MAXW][RT];
    __shared__ double red[4][WPW][RT];
    __shared__ int is_last;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t tile = blockIdx.x / geo.nsplit;
    const int split = (int)(blockIdx.x - tile * geo.nsplit);
    const int64_t row0 = tile * RT;
    const int lr = lane & 15, lg = lane >> 4;

    // which widths and which 16-column tiles of a chunk this wave owns
    int ncw, ct0, wi0;
    if (nw == 1) { ncw = 1; ct0 = wv; wi0 = 0; }
    else if (nw == 2) { ncw = 2; ct0 = 2 * (wv >> 1); wi0 = wv & 1; }
    else { ncw = 4; ct0 = 0; wi0 = wv; }

    // the tile's quantisers (a row beyond R repeats the last row: in bounds, never stored)
    for (int e = tid; e < nw * RT; e += 256) {
        const int i = e / RT, r = e - i * RT;
        const int64_t row = row0 + r < R ? row0 + r : R - 1;
        const int64_t pi = (int64_t)i * (per_row ? R : 1) + (per_row ? row : 0);
        ps[i][r] = scale[pi];
        pz[i][r] = rintf(zp[pi]);
    }
    __syncthreads();

    bool act[WPW], sig[WPW];
    float sa[WPW], za[WPW], qm[WPW];
    int wi[WPW];
#pragma unroll
    for (int j = 0; j < WPW; ++j) {
        wi[j] = wi0 + 4 * j;
        act[j] = wi[j] < nw;
        const int wc = act[j] ? wi[j] : 0;
        wi[j] = wc;
        sig[j] = wd.bits[wc] == 0;
        qm[j] = (float)((1 << wd.bits[wc]) - 1);
        sa[j] = ps[wc][lr];
        za[j] = pz[wc][lr];
    }

    // staging roles: H tile -- thread t loads 8 doubles of row t >> 3 at column 8 (t & 7); w tile -- elements t and t + 256 of 16 x 32
    const int hr = tid >> 3, hc = (tid & 7) * 8;
    const int wr0 = tid >> 5, wc0 = tid & 31;
    const int64_t wrow0 = row0 + wr0 < R ? row0 + wr0 : R - 1;
    const int64_t wrow1 = row0 + wr0 + 8 < R ? row0 + wr0 + 8 : R - 1;

    double rs[WPW][4];
#pragma unroll
    for (int j = 0; j < WPW; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) rs[j][i] = 0.0;

    const int c_begin = split * geo.cpw;
    const int c_end = c_begin + geo.cpw < geo.nchunks ? c_begin + geo.cpw : geo.nchunks;
    for (int ch = c_begin; ch < c_end; ++ch) {
        const int n0 = ch * CN;
        const bool hin = n0 + hc < K;                                   // (K is a multiple of 32: a thread's 8 columns are in or out)
        double4_t acc[WPW][4];
#pragma unroll
        for (int j = 0; j < WPW; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[j][c] = (double4_t){0.0, 0.0, 0.0, 0.0};

        double2 hv[4];
        float wf0, wf1;
        auto fetch = [&](int j0) {
            const double2* src = reinterpret_cast<const double2*>(H + (int64_t)(j0 + hr) * ldh + n0 + hc);
#pragma unroll
            for (int q = 0; q < 4; ++q) hv[q] = hin ? src[q] : make_double2(0.0, 0.0);
            wf0 = w[wrow0 * ldw + j0 + wc0];
            wf1 = w[wrow1 * ldw + j0 + wc0];
        };
        fetch(0);
        for (int j0 = 0; j0 < K; j0 += KB) {
            __syncthreads();                                            // the previous tile has been read
            double2* dst = reinterpret_cast<double2*>(Ht + hr * HLD + hc);
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[q] = hv[q];
            Wt[wr0 * WLD + wc0] = wf0;
            Wt[(wr0 + 8) * WLD + wc0] = wf1;
            __syncthreads();
            if (j0 + KB < K) fetch(j0 + KB);
#pragma unroll
            for (int s = 0; s < KB / 4; ++s) {
                const float wa = Wt[lr * WLD + 4 * s + lg];
                double b[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < ncw) b[c] = Ht[(4 * s + lg) * HLD + (ct0 + c) * 16 + lr];
#pragma unroll
                for (int j = 0; j < WPW; ++j) {
                    if (!act[j]) continue;
                    const double d = bc_d(wa, sa[j], za[j], qm[j], sig[j]);
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < ncw) acc[j][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(d, b[c], acc[j][c], 0, 0, 0);
                }
            }
        }
        // epilogue: register i of a lane is E[row lg + 4 i][column lr of its tile]; fold E * D into the lane's row sums
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int col = n0 + (ct0 + c) * 16 + lr;
            if (c < ncw && col < K) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = lg + 4 * i;
                    const int64_t row = row0 + r < R ? row0 + r : R - 1;
                    const float x = w[row * ldw + col];
#pragma unroll
                    for (int j = 0; j < WPW; ++j)
                        if (act[j]) {
                            const double d = bc_d(x, ps[wi[j]][r], pz[wi[j]][r], qm[j], sig[j]);
                            rs[j][i] = rs[j][i] + acc[j][c][i] * d;
                        }
                }
            }
        }
    }

    // the 16 lanes of a row (fixed butterfly), then the waves that share a width in wave order
#pragma unroll
    for (int j = 0; j < WPW; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double v = rs[j][i];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
            if (lr == 0) red[wv][j][lg + 4 * i] = v;
        }
    __syncthreads();
    double total = 0.0;
    const bool owner = tid < nw * RT;
    const int oi = tid / RT, orow = tid - oi * RT;
    if (owner) {
        if (nw == 1) total = ((red[0][0][orow] + red[1][0][orow]) + red[2][0][orow]) + red[3][0][orow];
        else if (nw == 2) total = red[oi][0][orow] + red[oi + 2][0][orow];
        else total = red[oi & 3][WPW > 1 ? oi >> 2 : 0][orow];
    }
    if (geo.nsplit == 1) {
        if (owner && row0 + orow < R) cost[(int64_t)oi * R + row0 + orow] = total;
        return;
    }
    double* mine = part + (tile * geo.nsplit + split) * (int64_t)(nw * RT);
    if (owner) __hip_atomic_store(mine + tid, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    fpcs::publish_wait();                                               // the partials are at the coherence point before the ticket
    __syncthreads();
    if (tid == 0) is_last = fpcs::ticket_last(tickets + tile, (unsigned)geo.nsplit) ? 1 : 0;
    __syncthreads();
    if (!is_last || !owner) return;
    const double* all = part + tile * geo.nsplit * (int64_t)(nw * RT) + tid;
    double sum = 0.0;
    for (int sp = 0; sp < geo.nsplit; ++sp)
        sum = sum + __hip_atomic_load(all + (int64_t)sp * (nw * RT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (row0 + orow < R) cost[(int64_t)oi * R + row0 + orow] = sum;
}

inline int64_t ws_bytes(const Geo& g, int nw) {
    if (g.nsplit <= 1) return 0;
    return part_doubles(g, nw) * (int64_t)sizeof(double) + ((g.tiles * (int64_t)sizeof(unsigned int) + 7) & ~(int64_t)7);
}

}  // namespace

extern "C" int adalog_bit_cost_ok(int64_t R, int64_t K, int n_widths) {
    return R >= 1 && R <= ((int64_t)1 << 31) && K >= 32 && K <= 4096 && K % 32 == 0 && n_widths >= 1 && n_widths <= MAXW;
}

extern "C" int64_t adalog_bit_cost_workspace_bytes(int64_t R, int64_t K, int n_widths) {
    if (!adalog_bit_cost_ok(R, K, n_widths)) return -1;
    return ws_bytes(bc_geo(R, K), n_widths);
}

extern "C" int adalog_bit_cost_f32(const float* w, int64_t R, int64_t K, int64_t ldw, const float* scale, const float* zero_point,
                                   int per_row, const int* bits, int n_widths, const double* H, int64_t ldh, double* cost,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    ADALOG_ARG_CHECK(adalog_bit_cost_ok(R, K, n_widths),
                     "bit_cost: unsupported sizes (R >= 1, K a multiple of 32 in [32, 4096], 1 <= n_widths <= 8)");
    ADALOG_ARG_CHECK(w && scale && zero_point && bits && H && cost, "bit_cost: null pointer");
    Widths wd;
    for (int i = 0; i < MAXW; ++i) wd.bits[i] = 0;
    for (int i = 0; i < n_widths; ++i) {
        ADALOG_ARG_CHECK(bits[i] == 0 || (bits[i] >= 2 && bits[i] <= 8), "bit_cost: a width must be 0 (the signal row) or in [2,8]");
        wd.bits[i] = bits[i];
    }
    ADALOG_ARG_CHECK(ldw >= K && ldh >= K, "bit_cost: bad sizes (ldw >= K, ldh >= K)");
    ADALOG_ARG_CHECK(per_row == 0 || per_row == 1, "bit_cost: per_row must be 0 or 1");
    ADALOG_ARG_CHECK(((uintptr_t)w & 3) == 0 && ((uintptr_t)H & 15) == 0 && ldh % 2 == 0 && ((uintptr_t)cost & 7) == 0,
                     "bit_cost: w must be 4-byte, cost 8-byte and H 16-byte aligned with an even ldh");
    const Geo g = bc_geo(R, K);
    const int64_t need = ws_bytes(g, n_widths);
    ADALOG_ARG_CHECK(need == 0 || (workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= need),
                     "bit_cost: workspace missing, misaligned or smaller than the workspace query's answer");
    hipStream_t st = (hipStream_t)stream;
    double* part = nullptr;
    unsigned int* tickets = nullptr;
    if (need) {
        part = (double*)workspace;
        tickets = (unsigned int*)(part + part_doubles(g, n_widths));
        const hipError_t e = hipMemsetAsync(tickets, 0, (size_t)g.tiles * sizeof(unsigned int), st);
        if (e != hipSuccess) { adalog_set_error("bit_cost: hipMemsetAsync", e); return (int)e; }
    }
    const dim3 grid((unsigned)(g.tiles * g.nsplit));
    int rc;
    if (n_widths <= 4)
        rc = adalog_launch<k_bit_cost<1>>("k_bit_cost", 0, grid, 256, 0, st, w, R, (int)K, ldw, scale, zero_point, per_row, wd, n_widths,
                                          H, ldh, cost, part, tickets, g);
    else
        rc = adalog_launch<k_bit_cost<2>>("k_bit_cost", 0, grid, 256, 0, st, w, R, (int)K, ldw, scale, zero_point, per_row, wd, n_widths,
                                          H, ldh, cost, part, tickets, g);
    if (rc) return rc;
    ADALOG_LAUNCH_CHECK("adalog_bit_cost_f32");
    return 0;
}
