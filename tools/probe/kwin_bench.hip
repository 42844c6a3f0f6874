// Standalone A/B harness for the fused window kernel (GPU box): compiles kwin.hpp (+ the k_win2 probe) without the
// rest of the library (seconds instead of a minute), runs each variant on the cfg3 shape (4096 windows x 8 buoys x
// 4096 samples, synthetic: a common random source with integer delays per buoy + noise), checks every integer lag
// against the generator's delays and compares the three output arrays of every variant bit for bit with variant 0.
// Not a parity test (that is tests/ through the C ABI against the oracle): a timing instrument whose kernels must
// at least agree with each other.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -mllvm -simplifycfg-sink-common=false \
//        [-DKWB_VARIANTS=...] -o kwin_bench kwin_bench.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../radio-mapper_amd/csrc/host_plan.hpp"
#include "../../radio-mapper_amd/csrc/kwin.hpp"
#if !defined(KWB_NO_KWIN2)
#include "kwin2.hpp"
#define KWB_HAVE_KWIN2 1
#endif
#if !defined(KWB_NO_P1)
#include "kwin_p1.hpp"
#endif
#if !defined(KWB_NO_FX)
#include "kwin_fx.hpp"
#endif

using namespace rmx;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

__host__ __device__ inline unsigned hash32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__host__ __device__ inline int delay_of(int w, int b) { return (int)(hash32(0x9e3779b9u * (unsigned)(w * 64 + b) + 12345u) % 201u) - 100; }
__device__ inline float unif(unsigned h) { return (float)(h >> 8) * (2.0f / 16777216.0f) - 1.0f; }

__global__ void k_gen(float2* iq, int B, int N) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;   // over W*B*N
    const int n = (int)(idx % N);
    const long wb = idx / N;
    const int b = (int)(wb % B), w = (int)(wb / B);
    const int m = n - delay_of(w, b);                                // x_b[n] = s[n - d_b]
    const unsigned hs = hash32((unsigned)w * 0x85ebca6bu + (unsigned)(m + 4096) * 0xc2b2ae35u + 1u);
    const unsigned hn = hash32((unsigned)idx * 0x27d4eb2fu + 77u);
    const float sr = unif(hs), si = unif(hash32(hs ^ 0xdeadbeefu));
    const float nr = unif(hn), ni = unif(hash32(hn ^ 0x1234567u));
    iq[idx] = make_float2(70.0f * sr + 25.0f * nr, 70.0f * si + 25.0f * ni);
}

struct Bufs {
    float2* iq; float4* spec; float4* tw1; float2* tw2; int4* trail; int* li; float* lf; float* pk;
    int W, B; float out_scale;
};

typedef void (*launch_fn)(const Bufs&, hipStream_t);

static void launch_base(const Bufs& b, hipStream_t s) {
    hipLaunchKernelGGL(k_win<false>, dim3(256), dim3(kThreads), kLdsWinBytes, s, (const void*)b.iq, b.spec, b.tw1, b.tw2, b.B, 0L,
                       b.out_scale, b.li, b.lf, b.pk, b.W, (const int4*)b.trail, 1);
}
static void launch_stag0(const Bufs& b, hipStream_t s) {
    hipLaunchKernelGGL(k_win<false>, dim3(256), dim3(kThreads), kLdsWinBytes, s, (const void*)b.iq, b.spec, b.tw1, b.tw2, b.B, 0L,
                       b.out_scale, b.li, b.lf, b.pk, b.W, (const int4*)b.trail, 0);
}
#ifdef KWB_HAVE_KWIN2
#define KWB_V2(NAME, ...)                                                                                               \
    static void NAME(const Bufs& b, hipStream_t s) {                                                                    \
        hipLaunchKernelGGL((k_win2<false, __VA_ARGS__>), dim3(256), dim3(kThreads), kLdsWin2Bytes, s, (const void*)b.iq, \
                           b.spec, b.tw1, b.tw2, b.B, 0L, b.out_scale, b.li, b.lf, b.pk, b.W);                          \
    }
KWB_V2(launch_2a, 1)
KWB_V2(launch_2a_s0, 0)
KWB_V2(launch_2a_l, 1, 0, true)
KWB_V2(launch_a1, 1, 1)
KWB_V2(launch_a4, 1, 4)
KWB_V2(launch_a8, 1, 8)
KWB_V2(launch_a15, 1, 15)
#define KWB_KWIN2_TABLE \
    {"k_win2 two anchors, STAG 1", launch_2a, (const void*)k_win2<false, 1>, kLdsWin2Bytes}, \
    {"k_win2 two anchors, STAG 0", launch_2a_s0, (const void*)k_win2<false, 0>, kLdsWin2Bytes}, \
    {"k_win2 two anchors, STAG 1, TW2 row from LDS", launch_2a_l, (const void*)k_win2<false, 1, 0, true>, kLdsWin2Bytes}, \
    {"k_win2 ABL 1: no spectrum loads (phase 2)", launch_a1, (const void*)k_win2<false, 1, 1>, kLdsWin2Bytes}, \
    {"k_win2 ABL 4: no spectrum stores", launch_a4, (const void*)k_win2<false, 1, 4>, kLdsWin2Bytes}, \
    {"k_win2 ABL 8: no sample prefetch", launch_a8, (const void*)k_win2<false, 1, 8>, kLdsWin2Bytes}, \
    {"k_win2 ABL 15: all", launch_a15, (const void*)k_win2<false, 1, 15>, kLdsWin2Bytes},
#endif

#if !defined(KWB_NO_P1)
// the request side of phase 1 (kwin_p1.hpp, LABNOTES R12): P1 bits 1 no store of X_{B-1}, 2 stores spread over the groups of
// h1, 4 priority for waves 4-7, 8 every store under a run-time mask that is false (timing only), 16 stores spread over four groups
#define KWB_P1(NAME, BITS)                                                                                                  \
    static void NAME(const Bufs& b, hipStream_t s) {                                                                         \
        hipLaunchKernelGGL((k_win_p1<false, BITS>), dim3(256), dim3(kThreads), kLdsWinBytes, s, (const void*)b.iq, b.spec,   \
                           b.tw1, b.tw2, b.B, 0L, b.out_scale, b.li, b.lf, b.pk, b.W, (const int4*)b.trail, 0, 0);           \
    }
KWB_P1(launch_p1_0, 0)
KWB_P1(launch_p1_8, 8)
KWB_P1(launch_p1_1, 1)
KWB_P1(launch_p1_2, 2)
KWB_P1(launch_p1_16, 16)
KWB_P1(launch_p1_4, 4)
KWB_P1(launch_p1_3, 3)
KWB_P1(launch_p1_5, 5)
KWB_P1(launch_p1_7, 7)
#define KWB_P1_TABLE \
    {"p1 0: the body before R12, stag 0", launch_p1_0, (const void*)k_win_p1<false, 0>, kLdsWinBytes}, \
    {"p1 8: stores masked at run time (TIMING ONLY)", launch_p1_8, (const void*)k_win_p1<false, 8>, kLdsWinBytes}, \
    {"p1 1: no store of X_{B-1}", launch_p1_1, (const void*)k_win_p1<false, 1>, kLdsWinBytes}, \
    {"p1 2: stores spread over eight groups", launch_p1_2, (const void*)k_win_p1<false, 2>, kLdsWinBytes}, \
    {"p1 16: stores spread over four groups", launch_p1_16, (const void*)k_win_p1<false, 16>, kLdsWinBytes}, \
    {"p1 4: priority in phase 1", launch_p1_4, (const void*)k_win_p1<false, 4>, kLdsWinBytes}, \
    {"p1 3: 1 + 2", launch_p1_3, (const void*)k_win_p1<false, 3>, kLdsWinBytes}, \
    {"p1 5: 1 + 4", launch_p1_5, (const void*)k_win_p1<false, 5>, kLdsWinBytes}, \
    {"p1 7: 1 + 2 + 4", launch_p1_7, (const void*)k_win_p1<false, 7>, kLdsWinBytes},
#endif

#if !defined(KWB_NO_FX)
// the forward transform's barrier exchange (kwin_fx.hpp, LABNOTES R17): FX bits 1 sixteen plain ds_read_b64 in fwd, 2 the
// forward-only image without the store conflict, 4 sixteen plain ds_write_b64 for role B's stores in h1, 8 / 16 / 32 see
// kwin_fx.hpp.  (k_win itself is what shipped, FX = 3; `fx 0` is the body before R17.)
#define KWB_FX(NAME, BITS)                                                                                                  \
    static void NAME(const Bufs& b, hipStream_t s) {                                                                         \
        hipLaunchKernelGGL((k_win_fx<false, BITS>), dim3(256), dim3(kThreads), kLdsWinBytes, s, (const void*)b.iq, b.spec,   \
                           b.tw1, b.tw2, b.B, 0L, b.out_scale, b.li, b.lf, b.pk, b.W, (const int4*)b.trail, 0);              \
    }
KWB_FX(launch_fx_0, 0)
KWB_FX(launch_fx_1, 1)
KWB_FX(launch_fx_2, 2)
KWB_FX(launch_fx_3, 3)
KWB_FX(launch_fx_4, 4)
KWB_FX(launch_fx_7, 7)
KWB_FX(launch_fx_9, 9)
KWB_FX(launch_fx_11, 11)
KWB_FX(launch_fx_19, 19)
KWB_FX(launch_fx_35, 35)
#define KWB_FX_TABLE \
    {"fx 0: the body before R17, stag 0", launch_fx_0, (const void*)k_win_fx<false, 0>, kLdsWinBytes}, \
    {"fx 1: A, plain reads in fwd", launch_fx_1, (const void*)k_win_fx<false, 1>, kLdsWinBytes}, \
    {"fx 2: B, forward-only image", launch_fx_2, (const void*)k_win_fx<false, 2>, kLdsWinBytes}, \
    {"fx 3: A + B", launch_fx_3, (const void*)k_win_fx<false, 3>, kLdsWinBytes}, \
    {"fx 4: plain role-B stores in h1", launch_fx_4, (const void*)k_win_fx<false, 4>, kLdsWinBytes}, \
    {"fx 7: A + B + plain stores", launch_fx_7, (const void*)k_win_fx<false, 7>, kLdsWinBytes}, \
    {"fx 9: A, values as opaque scalars", launch_fx_9, (const void*)k_win_fx<false, 9>, kLdsWinBytes}, \
    {"fx 11: A + B, values as opaque scalars", launch_fx_11, (const void*)k_win_fx<false, 11>, kLdsWinBytes}, \
    {"fx 19: A + B, bases computed per transform", launch_fx_19, (const void*)k_win_fx<false, 19>, kLdsWinBytes}, \
    {"fx 35: A + B, bases from the inverse's per transform", launch_fx_35, (const void*)k_win_fx<false, 35>, kLdsWinBytes},
#endif

struct Variant { const char* name; launch_fn fn; const void* kfn; int lds; };

int main(int argc, char** argv) {
    const int W = argc > 1 ? atoi(argv[1]) : 4096, B = argc > 4 ? atoi(argv[4]) : 8, N = kM;
    const int reps = argc > 2 ? atoi(argv[2]) : 200, warm = argc > 3 ? atoi(argv[3]) : 150;
    const int P = B * (B - 1) / 2;
    Bufs b{};
    b.W = W; b.B = B;
    {
        int logl = 0;
        while ((1 << logl) < kL) ++logl;
        b.out_scale = std::ldexp(1.0f, 3 * kTw1ScaleLog2 - logl);
    }
    CK(hipMalloc(&b.iq, (size_t)W * B * N * 8));
    CK(hipMalloc(&b.spec, (size_t)256 * B * 8 * kThreads * 16));
    CK(hipMalloc(&b.li, (size_t)W * P * 4)); CK(hipMalloc(&b.lf, (size_t)W * P * 4)); CK(hipMalloc(&b.pk, (size_t)W * P * 4));
    std::vector<float4> tw1; std::vector<float2> tw2;
    build_tables(tw1, tw2);
    CK(hipMalloc(&b.tw1, tw1.size() * 16)); CK(hipMalloc(&b.tw2, tw2.size() * 8));
    CK(hipMemcpy(b.tw1, tw1.data(), tw1.size() * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(b.tw2, tw2.data(), tw2.size() * 8, hipMemcpyHostToDevice));
    {   // the order of a window's pairs among buoys 1 .. B-1
        const host::PairTrail tr = host::plan_pair_trail(B);
        const std::vector<int32_t> e = host::encode_pair_trail(tr);
        if (e.empty()) { printf("the kernel cannot walk this pair order\n"); return 1; }
        CK(hipMalloc(&b.trail, e.size() * 4));
        CK(hipMemcpy(b.trail, e.data(), e.size() * 4, hipMemcpyHostToDevice));
        printf("pair order: %d steps, %d requests + 1 from phase 1, %d reloads, simulated hits LRU2 %d LRU3 %d\n", (int)tr.steps.size(),
               tr.loads, tr.reloads, tr.sim_hits2, tr.sim_hits3);
    }
    hipLaunchKernelGGL(k_gen, dim3((unsigned)((long)W * B * N / 256)), dim3(256), 0, 0, b.iq, B, N);
    CK(hipDeviceSynchronize());

    std::vector<Variant> vars = {
        {"k_win stag=1", launch_base, (const void*)k_win<false>, kLdsWinBytes},
        {"k_win stag=0 (production)", launch_stag0, (const void*)k_win<false>, kLdsWinBytes},
#ifdef KWB_HAVE_KWIN2
        KWB_KWIN2_TABLE
#endif
#ifdef KWB_P1_TABLE
        KWB_P1_TABLE
#endif
#ifdef KWB_FX_TABLE
        KWB_FX_TABLE
#endif
    };
    const int rounds = argc > 7 ? atoi(argv[7]) : 2;   // argv[7]: interleaved runs of every variant
    if (argc > 6 && argv[6][0] != '-') vars = {vars.at((size_t)atoi(argv[6]))};   // argv[6]: that variant alone (counter passes: one kernel name, one order); "-": all
    for (auto& v : vars) CK(hipFuncSetAttribute(v.kfn, hipFuncAttributeMaxDynamicSharedMemorySize, v.lds));

    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<int> li0, li((size_t)W * P);
    std::vector<float> lf0, pk0, lf((size_t)W * P), pk((size_t)W * P);
    const double alg_bytes = (double)W * P * (16.0 * N + 12.0);
    for (int round = 0; round < rounds; ++round)
        for (size_t vi = 0; vi < vars.size(); ++vi) {
            auto& v = vars[vi];
            CK(hipMemset(b.li, 0xff, (size_t)W * P * 4)); CK(hipMemset(b.lf, 0xff, (size_t)W * P * 4)); CK(hipMemset(b.pk, 0xff, (size_t)W * P * 4));
            for (int i = 0; i < (round ? 20 : warm); ++i) v.fn(b, 0);
            CK(hipDeviceSynchronize());
            CK(hipEventRecord(e0));
            for (int i = 0; i < reps; ++i) v.fn(b, 0);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            ms /= reps;
            CK(hipMemcpy(li.data(), b.li, li.size() * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(lf.data(), b.lf, lf.size() * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(pk.data(), b.pk, pk.size() * 4, hipMemcpyDeviceToHost));
            long bad_truth = 0, diff_li = 0, diff_lf = 0, diff_pk = 0;
            for (int w = 0; w < W; ++w) {
                int o = 0;
                for (int i = 0; i < B; ++i)
                    for (int j = i + 1; j < B; ++j, ++o)
                        if (li[(size_t)w * P + o] != delay_of(w, j) - delay_of(w, i)) ++bad_truth;
            }
            if (vi == 0 && round == 0) {
                li0 = li; lf0 = lf; pk0 = pk;
                if (argc > 5 && strcmp(argv[5], "-") != 0) {   // argv[5]: prefix of three raw files ("-": none), to set two builds of the harness against each other
                    const char* ext[3] = {".li", ".lf", ".pk"};
                    const void* src[3] = {li.data(), lf.data(), pk.data()};
                    for (int k = 0; k < 3; ++k) {
                        FILE* f = fopen((std::string(argv[5]) + ext[k]).c_str(), "wb");
                        if (f) { fwrite(src[k], 4, li.size(), f); fclose(f); }
                    }
                }
            }
            else
                for (size_t k = 0; k < li.size(); ++k) {
                    diff_li += li[k] != li0[k];
                    diff_lf += memcmp(&lf[k], &lf0[k], 4) != 0;
                    diff_pk += memcmp(&pk[k], &pk0[k], 4) != 0;
                }
            // FNV-1a over the three output arrays: two builds of the harness are compared through it
            unsigned long long hsum = 1469598103934665603ULL;
            auto fnv = [&](const void* ptr, size_t nb) {
                const unsigned char* c = (const unsigned char*)ptr;
                for (size_t k = 0; k < nb; ++k) { hsum ^= c[k]; hsum *= 1099511628211ULL; }
            };
            fnv(li.data(), li.size() * 4); fnv(lf.data(), lf.size() * 4); fnv(pk.data(), pk.size() * 4);
            printf("[%d] %-44s %.4f ms  frac %.4f | lags != generator %ld, vs variant 0: lag_int %ld lag_frac %ld peak %ld differ | fnv %016llx\n", round,
                   v.name, ms, alg_bytes / (ms * 1e-3) / 8e12, bad_truth, diff_li, diff_lf, diff_pk, hsum);
            fflush(stdout);
        }
    return 0;
}
