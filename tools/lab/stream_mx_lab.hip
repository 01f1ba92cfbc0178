// Lab harness (not product): k_gemm_stream<bf16xfp8> at the fc2 weight-search shape of deit_small (32 images), per-launch time and a
// hash of the partials.  Built once per ablation / schedule (make -C tools/lab stream_mx_labs); the table the builds give is
// profiles/stream_mx_ablation.txt.  Run on the GPU box: tools/lab/stream_mx_lab_<variant> [launches]
#include "../../adalog_amd/csrc/gemm_score.hip"
#include <vector>
#include <algorithm>
#include <string.h>

static char g_err[512];
extern "C" void adalog_set_error(const char* where, hipError_t e) { snprintf(g_err, sizeof g_err, "%s: %s", where, hipGetErrorString(e)); }
extern "C" void adalog_set_error_msg(const char* msg) { snprintf(g_err, sizeof g_err, "%s", msg); }
extern "C" void adalog_note_kernel(const char*) {}
// (the finish entry points of gemm_score.hip call into other translation units of the library; the lab calls none of them)
extern "C" unsigned int* adalog_ticket_slots_on(int, void*) { return nullptr; }
extern "C" int adalog_topk_next_tail(const float*, int, int, const adalog_fpcs_tail*, int*, void*) { return 1; }
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

#ifndef LAB_NAME
#define LAB_NAME "shipped"
#endif

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 40;
    const int M = 32 * 197, P = 128, O = 384, N = O * P, K = 1536;
    // A: bf16 AdaLog-like values 30 x 2^-t (t = 0 .. 15), B: the fp8 e4m3 encodings of the integers -8 .. 7
    static const uint8_t f8[16] = {0xD0, 0xCE, 0xCC, 0xCA, 0xC8, 0xC4, 0xC0, 0xB8, 0x00, 0x38, 0x40, 0x44, 0x48, 0x4A, 0x4C, 0x4E};
    std::vector<uint16_t> ha((size_t)M * K);
    for (size_t i = 0; i < ha.size(); ++i) ha[i] = (uint16_t)(0x41F0 - 0x80 * ((unsigned)(i * 2654435761u >> 13) & 15));
    std::vector<uint8_t> hb((size_t)N * K);
    for (size_t i = 0; i < hb.size(); ++i) hb[i] = f8[(unsigned)(i * 40503u >> 7) & 15];
    std::vector<float> hr((size_t)M * O);
    for (size_t i = 0; i < hr.size(); ++i) hr[i] = (float)((int)((i * 2246822519u >> 11) & 255) - 128) * 0.25f;
    std::vector<float> hs((size_t)N), hbias((size_t)O);
    for (size_t i = 0; i < hs.size(); ++i) hs[i] = 0.01f + 0.001f * (float)(i % 37);
    for (size_t i = 0; i < hbias.size(); ++i) hbias[i] = 0.125f * (float)(i % 11);
    uint8_t *A, *B; float *ref, *sa, *sb, *bias, *partial;
    CK(hipMalloc(&A, ha.size() * 2)); CK(hipMalloc(&B, hb.size()));
    CK(hipMemcpy(A, ha.data(), ha.size() * 2, hipMemcpyHostToDevice)); CK(hipMemcpy(B, hb.data(), hb.size(), hipMemcpyHostToDevice));
    CK(hipMalloc(&ref, hr.size() * 4)); CK(hipMemcpy(ref, hr.data(), hr.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&sa, 4)); CK(hipMalloc(&sb, hs.size() * 4)); CK(hipMalloc(&bias, hbias.size() * 4));
    CK(hipMemcpy(sa, hs.data(), 4, hipMemcpyHostToDevice)); CK(hipMemcpy(sb, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(bias, hbias.data(), hbias.size() * 4, hipMemcpyHostToDevice));
    if (!adalog_gemm_mixed_ok(M, N, 1, 1, P, K)) { printf("not a shape of the mixed streaming route\n"); return 1; }
    int MT, Npad, mode;
    const int64_t pe = adalog_gemm_score_layout(M, N, 1, 1, 1, P, 0, 4, K, K, 1, &MT, &Npad, &mode);
    CK(hipMalloc(&partial, pe * 4)); CK(hipMemset(partial, 0, pe * 4));
    auto run = [&]() {
        // the weight search's call: sb [P][O], bias per output column, transposed reference [O][M], per-column partials
        const int rc = adalog_gemm_score(4, A, B, 0, 0, 0, 0, M, N, K, K, 1, 1, 1, ref, 1, 0, M, P, sa, 0, 0, 0.5f, sb, O, 0, 1, bias, 0, 0, 1,
                                         nullptr, nullptr, partial, pe, nullptr, 0, 0, 0, 2, 0, nullptr);
        if (rc) { printf("gemm error: %s\n", g_err); exit(1); }
    };
    for (int i = 0; i < 3; ++i) run();
    CK(hipDeviceSynchronize());
    // per launch: one event pair each, so that the spread shows
    std::vector<hipEvent_t> ev(reps + 1);
    for (auto& e : ev) CK(hipEventCreate(&e));
    CK(hipEventRecord(ev[0]));
    for (int i = 0; i < reps; ++i) { run(); CK(hipEventRecord(ev[i + 1])); }
    CK(hipEventSynchronize(ev[reps]));
    std::vector<float> us(reps);
    for (int i = 0; i < reps; ++i) { CK(hipEventElapsedTime(&us[i], ev[i], ev[i + 1])); us[i] *= 1e3f; }
    std::sort(us.begin(), us.end());
    double mean = 0; for (float u : us) mean += u; mean /= reps;
    std::vector<uint32_t> hp((size_t)pe);
    CK(hipMemcpy(hp.data(), partial, hp.size() * 4, hipMemcpyDeviceToHost));
    uint64_t h = 1469598103934665603ull;
    for (uint32_t v : hp) { h ^= v; h *= 1099511628211ull; }
    const double flop = 2.0 * M * (double)N * K;
    printf("%-28s MT %d  %d launches: mean %8.1f us  median %8.1f  min %8.1f  max %8.1f  | %6.1f TFLOP/s (median)  partials %016llx\n", LAB_NAME, MT,
           reps, mean, us[reps / 2], us[0], us[reps - 1], flop / us[reps / 2] * 1e-6, (unsigned long long)h);
    return 0;
}
