// rmx_hip.hip -- the host side and the C ABI (include/rmx.h) of the TDoA cross-correlation engine; every kernel it
// launches lives in a header of this directory.
//
// Path (conventions of tdoa_processor.py:20,51,156-157,166-170):
//   per window w, pair (i<j):  r = IFFT_L( FFT_L(x_j) * conj(FFT_L(x_i)) ), L = 2N (zero padded)
//                               m = |r|, k = argmax over the 2N-1 'full' lags, parabolic offset.
// N = 4096 runs the fused kernel k_win (kwin.hpp) or, per chunk of windows on one stream, the two families of
// pair4096.hpp: k_fwd (forward spectra -> HBM/L2 scratch) and k_pair_* (product, inverse transform, peak search).  The
// other lengths run generic_path.hpp / win_eo.hpp / kwin8k.hpp / kwin16k.hpp.  host_plan.hpp chooses among them per
// call; every launch goes through rmx::launch below.  The generic path's thread counts, its four-step split and the
// dynamic-LDS bytes of its launches are not computed here: generic_init asks gen::make_geometry (gen_geometry.hpp, the
// header the kernels take their LDS layouts from) once and keeps the answer in rmx_ctx::geo.
// No MFMA (not a contraction), no library FFT: every kernel is hand written for wave64 / LDS.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rmx.h"
#include "dev_buf.hpp"
#include "host_plan.hpp"
#include "host_request.hpp"
#include "lag_bounds.hpp"
#include "xspec_weight.hpp"
#include "xspec_bands.hpp"
#include "integrate.hpp"
#include "refine.hpp"
#include "quality.hpp"
#include "fft_r16.hpp"
#include "kwin.hpp"
#include "fft_r8.hpp"
#ifdef RMX_EXPERIMENTS   // k_win8 / k_winp: two other builds of the fused kernel, measured slower (tools/experiments/README.md)
#include "../../tools/experiments/win8.hpp"
#include "../../tools/experiments/winpk.hpp"
#endif
#include "generic_path.hpp"
#include "win_eo.hpp"
#include "pair4096.hpp"                         // N = 4096 per transform: k_fwd, k_pair_res, k_pair_str
#include "kwin8k.hpp"                           // N = 8192 on k_win's network, one anchor half resident in LDS (k_win8kl)
#include "kwin16k.hpp"                          // N = 16384 on the same network: four quarter transforms, two kernels (k16_fwd, k16_pairs)
#ifdef RMX_EXPERIMENTS
#include "../../tools/experiments/kwin8k.hpp"   // its two predecessors: parity-green, not faster (LABNOTES.md R4.6)
#endif
#include "caf_select.hpp"
#include "solve_path.hpp"
#include "detect_path.hpp"

namespace rmx {

// dev_buf.hpp's memory calls on HIP.  A refused request becomes the ctx's error text; its code is RMX_E_HIP (RMX_MEM).
struct HipMem {
    const hipStream_t* stream;   // the ctx's, as it is at the moment of the wait (rmx_set_stream)
    std::string* err;
    hipError_t last = hipSuccess;
    void* keep(void* p) {
        if (last == hipSuccess) return p;
        (void)hipGetLastError();
        return nullptr;
    }
    void* alloc(size_t bytes) { void* p = nullptr; last = hipMalloc(&p, bytes); return keep(p); }
    void free(void* p) { (void)hipFree(p); }
    void* alloc_pinned(size_t bytes) { void* p = nullptr; last = hipHostMalloc(&p, bytes, hipHostMallocDefault); return keep(p); }
    void free_pinned(void* p) { (void)hipHostFree(p); }
    bool upload(void* dst, const void* src, size_t bytes) { last = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); return last == hipSuccess; }
    void wait() { (void)hipStreamSynchronize(*stream); }
    void refused(const char* what, size_t bytes) {
        char buf[256];
        snprintf(buf, sizeof buf, "%s of %zu bytes failed: %s", what, bytes, hipGetErrorString(last));
        *err = buf;
    }
};
using Mem = mem::Arena<HipMem>;
template <class T> using Counted = mem::Buf<T, HipMem, mem::kCounted>;       // in rmx_scratch_bytes
template <class T> using Uncounted = mem::Buf<T, HipMem, mem::kUncounted>;   // not in it (the split is historical)
template <class T> using Pinned = mem::Buf<T, HipMem, mem::kPinned>;
template <class T, class Key> using Keyed = mem::Keyed<T, HipMem, Key>;      // uncounted, cached under Key

}  // namespace rmx

struct rmx_ctx {
    template <class T> using Counted = rmx::Counted<T>;
    template <class T> using Uncounted = rmx::Uncounted<T>;
    // a small host array that kernels read: staged through pinned memory into a ctx-owned device buffer (stage_to_device)
    struct DevStage {
        explicit DevStage(rmx::Mem* m) : h(m), d(m) {}
        rmx::Pinned<int32_t> h;
        Counted<int> d;
        hipEvent_t ev = nullptr;   // the last copy out of h: the next call waits for it before it rewrites h
    };
    struct PlanKey {   // what the pair plan on the device was built from
        std::vector<int32_t> pairs;
        int ppb = 0;
        bool operator==(const PlanKey& o) const { return ppb == o.ppb && pairs == o.pairs; }
    };
    // The generic path's kernels as rmx::pick_generic_kernels chose them for this ctx: one typed pointer per signature
    // (the template arguments below only name the signature), null = this ctx does not have that kernel.
    struct GenericKernels {
        decltype(&rmx::gen::g_cols_inv<4>) cols_inv = nullptr;
        decltype(&rmx::gen::g_cols_inv<4, 0, rmx::LagBounds>) cols_inv_lb = nullptr;                    // its bounded instantiation (rmx_xcorr_batch_bounded)
        decltype(&rmx::gen::g_cols_inv<4, 0, rmx::LagBounds, rmx::Integrate>) cols_inv_int = nullptr;   // its integrating one (integrate.hpp)
        decltype(&rmx::gen::g_cols_inv<4, 0, rmx::LagBounds, rmx::Integrate, rmx::BandSet>) cols_inv_int_bs = nullptr;   // ... behind the banded inverse rows
        decltype(&rmx::gen::g_cols_fwd<false, 4>) cols_fwd[2] = {nullptr, nullptr};                     // [u8]
        decltype(&rmx::gen::g_rows<true, false>) rows_fwd = nullptr;   // g_rows compiled for this row length (or the run-time one)
        decltype(&rmx::gen::g_rows<true, false, false, 0, rmx::XWeight>) rows_fwd_wt = nullptr;         // its weighted instantiation
        decltype(&rmx::gen::g_rows<false, true, true>) rows_inv = nullptr;
        decltype(&rmx::gen::g_rows<false, true, true, 0, rmx::BandSet>) rows_inv_bs = nullptr;          // its banded instantiation (rmx_xcorr_batch_bands)
        decltype(&rmx::gen::g_rows_anchor<9>) rows_anchor = nullptr;   // inverse rows with a resident anchor (default pair list)
        decltype(&rmx::gen::g_rows_fused<2, 9>) fused = nullptr;       // four-step: both row passes in one kernel (n_buoys <= 4)
        decltype(&rmx::gen::g_rows_fused<2, 9>) fused_def = nullptr;   // the same for the default plan (pair loop unrolled)
        decltype(&rmx::gen::g_win_fused<2, 9, false, false>) wf[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [default plan][u8]
        decltype(&rmx::gen::g_win_scr<9, false>) ws[2] = {nullptr, nullptr};    // [u8]: g_win_scr<log2 L> or g_win_scr14
        decltype(&rmx::gen::g_win_eo15<false>) ws15[2] = {nullptr, nullptr};    // [u8]: N = 16384 (one more table)
        size_t ws_lds = 0;                                                      // of ws or ws15, whichever is there
        int ws_thr = 0, ws_upw = 0;                                             // its threads and windows per workgroup
    };

    hipStream_t stream = nullptr;
    std::string err;
    rmx::Mem mem{{&stream, &err}};   // every buffer below allocates through it; mem.ledger is rmx_scratch_bytes
    rmx::host::Knobs knobs;   // kernel-selection options as they were at rmx_create (host_plan.hpp)
    int device = 0;
    int n_cus = 256;   // compute units of the device (persistent-grid size of the fused kernel)
    int n_buoys = 0, n_samples = 0, max_windows = 0;
    bool own_stream = false;
    int chunk_windows = 0;
    int pairs_per_block = 7;
    bool ppb_user = false;  // set through rmx_set_option: the small-batch rule then leaves it alone
    bool small_batch = true; // option small4096: few windows of N = 4096 through the per-transform kernels (see rmx_xcorr_batch)
    bool timing = false;
    bool resident = true;
    int pk = 0;             // fused path: 1 = k_winp (k_win on packed fp32)
    int win8 = 0;           // fused path: 1 = k_win8 (8 points x 1024 threads, 4 waves/SIMD), 0 = k_win
    int stag = 1;           // k_win8: which waves run the two halves between barriers in the opposite order
    int stag_kwin = 0;      // k_win / k_win_lb: the same choice; 0 (nobody) measured best since h1 stands once between two copies of h2 (LABNOTES R10.2)
    Counted<float4> d_tw1_8{&mem};
    Counted<float2> d_tb8{&mem}, d_tc8{&mem};
    bool fused = true;      // one kernel per chunk: forward spectra + pairs in one workgroup per window   // pair kernel variant: 1 workgroup/CU with resident tables
    // device buffers
    Counted<float4> d_spec{&mem}, d_tw1{&mem};
    Counted<float2> d_tw2{&mem};
    Counted<int32_t> d_trail{&mem};   // k_win: the order of a window's pairs among buoys 1 .. B-1 (host::plan_pair_trail), as int4
    rmx::Keyed<rmx::PairItem, PlanKey> d_items{&mem};   // the pair plan: both hold the same key, or the plan is not there
    rmx::Keyed<int, PlanKey> d_part_begin{&mem};
    Uncounted<char> d_in{&mem};
    Uncounted<float> d_out{&mem};       // ONE block of a host-pointer call's results: lag | frac | peak | dop (out_block)
    Uncounted<float> d_quality{&mem};   // rmx_xcorr_batch_quality's fourth output of a host-pointer call
    rmx::Pinned<char> h_out{&mem};      // pinned staging of small host-pointer results (fetch_out)
    // generic path (n_samples != 4096): see generic_path.hpp
    bool generic = false;
    rmx::gen::Geometry geo;    // lengths, split, thread counts and LDS bytes of every launch (gen_geometry.hpp), fixed by generic_init
    int g_chunk = 0;
    GenericKernels gk;
    bool g_fused = false;      // four-step: both row passes in g_rows_fused (n_buoys <= 4, plain batches)
    bool g_fused_always = false;
    bool g_wfused = false;     // LDS-resident lengths, n_buoys <= 4: whole windows in g_win_fused (no spectra in HBM)
    bool g_wscr = false;       // 512 <= L <= 16384, any buoy count: whole windows in g_win_scr (spectra in a cache-resident scratch)
    bool g_wscr_always = false;
    int g_ws_grid = 0;
    Counted<float4> g_ws_scratch{&mem};
    Counted<float2> g_tw_win{&mem};        // W_L half table of that kernel
    Counted<float2> g_tw_l{&mem};          // g_win_eo15 (N = 16384): W_32768^i, i < 1024
    bool g_k8 = false;                     // N = 8192: k_win8kl (kwin8k.hpp) instead of g_win_scr14 for batches that fill the chip
    int g_k8_kind = 1;                     // 1 = k_win8kl (LDS-resident anchor half), 2 = k_win8k (experiments build)
    Counted<float4> g_k8_tw1{&mem};        // its TW1 tables (both halves)
    Counted<float2> g_k8_tw2{&mem};        // k_win's TW2 table
    int g_k16 = 0;                         // N = 16384: k16_fwd + k16_pairs (kwin16k.hpp); 1 = from the measured batch size on, 2 = always
    Counted<float4> g_k16_tw1{&mem};       // slot factors of TW1
    Counted<float2> g_k16_gq{&mem}, g_k16_tw2{&mem}, g_k16_tws{&mem};   // per-quarter thread factors, k_win's TW2, W_128 rows
    int g_rows_anchor_min_b = 6;           // gk.rows_anchor from this many buoys on (option rows_anchor = n sets it, 0 = never)
    Counted<float2> g_tw{&mem}, g_tw1{&mem}, g_tw2{&mem}, g_thi{&mem}, g_tlo{&mem};
    // the chunk-sized buffers (generic_ensure): spectra, de-rotated spectra (CAF), products
    Counted<float2> g_spec{&mem}, g_spec_r{&mem}, g_prod{&mem};
    Counted<rmx::gen::GTile> g_rec{&mem};   // per column tile: partial argmax + taps
    Counted<float> g_halo{&mem};            // per column tile: |r|^2 of its two edge columns
    rmx::Keyed<rmx::gen::GPair, std::vector<int32_t>> g_pairs{&mem};   // under the plan's pair list
    // host-pointer input of the fused path: copies pipelined against the kernels on a second stream
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // rmx_detect_batch: twiddle table of the last window length, dB spectra, staging
    rmx::Keyed<float2, int> dt_tw{&mem};   // under log2 of the window length
    Uncounted<float> dt_pdb{&mem};
    Uncounted<char> dt_in{&mem}, dt_out{&mem};   // (dt_out: ONE block, bin | power | snr | confidence | count | floor)
    // rmx_solve_batch work buffers
    Uncounted<double> sv_buoys{&mem};
    Uncounted<int> sv_pairs{&mem};
    Uncounted<char> sv_in{&mem}, sv_out{&mem};   // ONE block each: lag_int | lag_frac | weight, pos | cost | iters
    // CAF (rmx_caf_batch): de-rotated spectra of the N = 4096 path, phasor table, per-hypothesis results
    Uncounted<float4> d_spec_r{&mem};
    rmx::Keyed<float2, std::vector<double>> caf_rot{&mem};   // under the Doppler grid
    Uncounted<int> caf_lag{&mem};
    Uncounted<float> caf_frac{&mem}, caf_peak{&mem};
    Uncounted<float> caf_nb{&mem};   // rmx_caf_batch_request with dop_frac: [3][slots] neighbour peaks of k_caf_select_fd,
                                     // then [slots] dop_frac of a host-pointer call
    // the caller's lag windows (rmx_xcorr_batch_bounded) and its bands as signed bins (rmx_xcorr_batch_weighted): the
    // device copies that a call's XcorrCall points into (rmx_xcorr_batch_bands: the full band, then the band set)
    DevStage lb_stage{&mem}, band_stage{&mem};
    // k_refine's and k_quality's pair list (refine.hpp): the plan's pairs in output order, under that list
    rmx::Keyed<rmx::RefPair, std::vector<int32_t>> rf_pairs{&mem};
    // the pair plan that d_items and d_part_begin hold (build_plan)
    std::vector<int32_t> plan_pairs;
    int plan_n_parts = 0;
    bool plan_all_pairs = false;   // the plan is the default list: all i<j in nested-loop order
    // timing
    std::vector<hipEvent_t> ev;
    std::vector<int> ev_kind;  // 0 fwd, 1 pair (per launch: ev[2k], ev[2k+1])
    size_t ev_used = 0;
    float t_fwd = 0, t_pair = 0;
    int n_fwd = 0, n_pair = 0;
};

namespace rmx {

using DevStage = rmx_ctx::DevStage;
using GenericKernels = rmx_ctx::GenericKernels;

static thread_local std::string g_create_error;

// What ONE correlation call asks of the launch code beyond the plain call: built by the entry (xcorr_request), handed
// down by const reference to every function that launches a kernel, never stored.  The default is the plain, unrefined
// call; rmx_caf_batch passes exactly that, rmx_caf_batch_request its bounds and its weighting.
struct XcorrCall {
    LagBounds lb{nullptr, 0, 0, 0};          // lag intervals on the device (rmx_xcorr_batch_bounded), or none
    XWeight wt{nullptr, 0, 0, 0, 0, 0.0f};   // bands as signed bins on the device + weighting (rmx_xcorr_batch_weighted)
    BandSet bs{nullptr, 0, 0, 1};            // several bands per window on the device (rmx_xcorr_batch_bands): the pair kernels
                                             // then walk n_bands virtual windows per window, lb and the outputs are per virtual
                                             // window, and wt is the full band (PHAT) or none
    int integ = 1;                           // windows per group (rmx_xcorr_batch_integrated): the bounds and the outputs
                                             // are then per GROUP, the bands stay per window, a chunk holds whole groups;
                                             // with bs (rmx_xcorr_batch_bands_integrated) per row group * n_bands + band
    int refine = 0;                          // U of rmx_xcorr_batch_refined: k_refine behind every chunk's pair kernels, or 0
    bool bounded() const { return lb.b != nullptr; }         // the bounded instantiations of the peak-searching kernels
    bool integrated() const { return integ > 1; }            // the integrating instantiations of the pair kernels
    bool banded() const { return bs.bins != nullptr; }       // the banded instantiations of the kernels that form the product
    float* quality = nullptr;                // rmx_xcorr_batch_quality: [rows][n_pairs][4] on the device (k_quality behind every
                                             // chunk's pair kernels, in front of k_refine), or none
    bool refined() const { return refine > 0; }              // k_refine reads both spectra of a pair from HBM
    bool qualified() const { return quality != nullptr; }    // k_quality does too
    // only the per-transform routes can serve it
    bool weighted() const { return wt.band != nullptr || bs.bins != nullptr || integ > 1 || refine > 0 || quality != nullptr; }
};

// Where a ctx's per-transform spectra lie once a chunk's forward kernels have run, and the launchers that write and read
// them (N = 4096: k_fwd / k_pair_*; generic: g_fwd_small / g_pair_small or the four-step passes).  Filled by spec_view().
struct SpecView {
    int layout;  const void* base;          // RefLayout (refine.hpp); d_spec / g_spec
    int logL, row_bits, unit_log2;          // log2 of the transform length; kRefRows: log2 of the rows per spectrum; the stored bins carry 2^unit_log2
    // rows_fused: four-step, g_rows_fused does both row passes (forward: the column pass only)
    int (*forward)(rmx_ctx*, const XcorrCall&, const void* d_iq, int w0, int wc, bool u8, const float2* rot, bool rows_fused);
    int (*pairs)(rmx_ctx*, const XcorrCall&, int w0, int wc, int n_pairs, int* d_lag, float* d_frac, float* d_peak, bool use_rot,
                 bool rows_fused);
};

// U8 as a compile-time constant: f(std::true_type) or f(std::false_type); returns what f returns
template <class F>
static auto with_u8(bool u8, F&& f) {
    if (u8) return f(std::true_type{});
    return f(std::false_type{});
}
// v as a compile-time constant: f(std::integral_constant<int, V>{}) for the V of the list that equals v; a v that is not
// in the list gets the LAST V (every table below names its fallback there).  Returns what f returns, one type for all V.
template <int V0, int... Vs, class F>
static auto with_one_of(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) {
        return f(std::integral_constant<int, V0>{});
    } else {
        if (v == V0) return f(std::integral_constant<int, V0>{});
        return with_one_of<Vs...>(v, f);
    }
}

static int fail(rmx_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

#define RMX_HIP(c, call)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail((c), RMX_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),    \
                        __FILE__, __LINE__);                                                      \
    } while (0)
// a buffer request (dev_buf.hpp: reserve, assign, refill) that failed: HipMem::refused has written the ctx's error text
#define RMX_MEM(ok)                    \
    do {                               \
        if (!(ok)) return RMX_E_HIP;   \
    } while (0)

using host::is_pow2;


#ifdef RMX_EXPERIMENTS
// tables of k_win8 (win8.hpp; the same values tools/model_win8.py checks against numpy's FFT)
static void build_tables8(std::vector<float4>& tw1, std::vector<float2>& tb, std::vector<float2>& tc) {
    const double two_pi = 6.283185307179586476925286766559;
    tw1.resize(4 * w8::kT8);
    for (int T = 0; T < w8::kT8; ++T) {
        const int p = T & 1, t1 = T >> 1;
        float2 w[8];
        for (int c0 = 0; c0 < 8; ++c0) {
            double ang = -two_pi * (double)((t1 * c0) % kM) / (double)kM;      // W_M^(c0 t1)
            if (p) ang += -two_pi * (double)t1 / (double)kL;                    // * W_L^t1 on odd lanes
            w[c0] = make_float2((float)(std::cos(ang) * kTw1Scale), (float)(std::sin(ang) * kTw1Scale));
        }
        for (int j = 0; j < 4; ++j) tw1[j * w8::kT8 + T] = make_float4(w[2 * j].x, w[2 * j].y, w[2 * j + 1].x, w[2 * j + 1].y);
    }
    // rows in the order the first butterfly layer consumes them: w4, w1, w5, w2, w6, w3, w7 (w0 = 1 not stored)
    const int order[7] = {4, 1, 5, 2, 6, 3, 7};
    auto fill = [&](std::vector<float2>& t, int rows, int n) {
        t.assign((size_t)rows * w8::kRowF2, make_float2(0.0f, 0.0f));
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < 7; ++k) {
                const double ang = -two_pi * (double)((r * order[k]) % n) / (double)n;
                t[(size_t)r * w8::kRowF2 + k] = make_float2((float)std::cos(ang), (float)std::sin(ang));
            }
    };
    fill(tb, 64, 512);   // W_512^(c1 * lane), lane = n0 + 8 n1
    fill(tc, 8, 64);     // W_64^(d0 * n0)
}
#endif

static int ensure_events(rmx_ctx* c, size_t n) {
    while (c->ev.size() < n) {
        hipEvent_t e;
        RMX_HIP(c, hipEventCreate(&e));
        c->ev.push_back(e);
    }
    return RMX_OK;
}

// Per-launch timing (option "timing"): every kernel launch of a call is bracketed by two HIP events on the launch stream
// and tagged with its kernel family; rmx_last_timing / rmx_last_timing_kind read them back.  The event pool grows in
// front of every record (a budget computed ahead of the chunk loop was too small once every chunk could take
// the partial-round route), so no call pattern can index past it.
enum TimeKind {
    kTkNone = -1,        // launch(): no record (k_solve, the detection kernels)
    kTkFwd4096 = 0,      // k_fwd
    kTkPair4096 = 1,     // k_win (fused forward + pairs) or k_pair_res / k_pair_str
    kTkColsFwd = 2,      // g_cols_fwd
    kTkRowsFwd = 3,      // g_rows (forward)
    kTkRowsFused = 4,    // g_rows_fused (forward rows, products, inverse rows)
    kTkRowsAnchor = 5,   // g_rows_anchor
    kTkRowsInv = 6,      // g_rows (product, inverse)
    kTkColsInv = 7,      // g_cols_inv
    kTkFinal = 8,        // g_final
    kTkWindow = 9,       // g_win_fused / g_win_scr / g_win_scr14 / g_win_eo15: whole windows in one kernel
    kTkFwdSmall = 10,    // g_fwd_small
    kTkPairSmall = 11,   // g_pair_small
    kTkCafSelect = 12,   // k_caf_select / k_caf_select_all
    kTkFwd16k = 13,      // k16_fwd
    kTkPairs16k = 14,    // k16_pairs
    kTkRefine = 15,      // k_refine
    kTkQuality = 16,     // k_quality
    kTkCount = 17
};
static const char* const kTimeKindName[kTkCount] = {
    "k_fwd", "k_win|k_pair", "g_cols_fwd", "g_rows_fwd", "g_rows_fused", "g_rows_anchor", "g_rows_inv", "g_cols_inv",
    "g_final", "g_win_*", "g_fwd_small", "g_pair_small", "k_caf_select", "k16_fwd", "k16_pairs", "k_refine",
    "k_quality"};
static int tm_begin(rmx_ctx* c) {
    if (!c->timing) return RMX_OK;
    const int rc = ensure_events(c, c->ev_used + 2);
    if (rc != RMX_OK) return rc;
    RMX_HIP(c, hipEventRecord(c->ev[c->ev_used], c->stream));
    return RMX_OK;
}
static int tm_end(rmx_ctx* c, int kind) {
    if (!c->timing) return RMX_OK;
    RMX_HIP(c, hipEventRecord(c->ev[c->ev_used + 1], c->stream));
    c->ev_used += 2;
    c->ev_kind.push_back(kind);
    return RMX_OK;
}
static void tm_reset(rmx_ctx* c) {
    c->ev_used = 0;
    c->ev_kind.clear();
}

// THE kernel launch: kern on c->stream with args converted to its parameter types P... (a wrong count or an
// inconvertible argument does not compile), bracketed by the timing record of family `kind` (kTkNone: none).  A launch
// the runtime refuses -- a null kern included -- is RMX_E_HIP under the family's name.
template <class... P, class... A>
static int launch(rmx_ctx* c, int kind, void (*kern)(P...), dim3 grid, dim3 block, size_t lds, A&&... args) {
    static_assert(sizeof...(P) == sizeof...(A), "launch: one argument per kernel parameter");
    const char* family = kind == kTkNone ? "kernel" : kTimeKindName[kind];
    if (!kern) return fail(c, RMX_E_HIP, "%s: this ctx has no such kernel", family);
    if (kind != kTkNone) {
        const int rc = tm_begin(c);
        if (rc != RMX_OK) return rc;
    }
    const hipError_t e = [&](P... p) {
        void* ptrs[] = {(void*)&p...};
        return hipLaunchKernel((const void*)kern, grid, block, ptrs, lds, c->stream);
    }(std::forward<A>(args)...);
    if (e != hipSuccess) {   // (the launch's own code: the runtime's last-error slot is read only to clear it)
        (void)hipGetLastError();
        return fail(c, RMX_E_HIP, "%s launch failed: %s", family, hipGetErrorString(e));
    }
    return kind == kTkNone ? RMX_OK : tm_end(c, kind);
}

// lets each of `kern` (typed kernel pointers; a null one is skipped) use `bytes` of dynamic LDS
template <class... P>
static const void* kernel_handle(void (*kern)(P...)) { return (const void*)kern; }
template <class... K>
static int allow_lds(rmx_ctx* c, size_t bytes, K... kern) {
    for (const void* k : {kernel_handle(kern)...})
        if (k) RMX_HIP(c, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return RMX_OK;
}

// pair plan (host_plan.hpp: validation, anchor runs, parts of <= pairs_per_block consecutive items) -> device copies
static int build_plan(rmx_ctx* c, const int32_t* pairs, int n_pairs) {
    host::PairPlan pp;
    std::string why;
    if (host::make_pair_plan(c->n_buoys, pairs, n_pairs, c->pairs_per_block, &pp, &why) != 0) return fail(c, RMX_E_INVAL, "%s", why.c_str());
    const rmx_ctx::PlanKey key{std::move(pp.pairs), c->pairs_per_block};
    if (c->d_items.holds(key) && c->d_part_begin.holds(key)) return RMX_OK;
    RMX_MEM(c->d_items.refill(key, pp.items.data(), (size_t)n_pairs));
    RMX_MEM(c->d_part_begin.refill(key, pp.part_begin.data(), (size_t)(pp.n_parts + 1)));
    c->plan_all_pairs = pp.all_pairs;
    c->plan_pairs = key.pairs;
    c->plan_n_parts = pp.n_parts;
    return RMX_OK;
}

// the plan's pairs in output order on the device, for the kernels that take one output slot per workgroup
static int ensure_ref_pairs(rmx_ctx* c, int n_pairs) {
    static_assert(sizeof(RefPair) == 2 * sizeof(int32_t), "a RefPair is one (i, j) of the plan's list");
    if (!c->rf_pairs.holds(c->plan_pairs))
        RMX_MEM(c->rf_pairs.refill(c->plan_pairs, reinterpret_cast<const RefPair*>(c->plan_pairs.data()), (size_t)n_pairs));
    return RMX_OK;
}

// The fine lag search of a refined call (refine.hpp) on the chunk the pair kernels have just finished: windows
// [w0, w0 + wc), whose spectra `spec` still holds in the order `layout` names.  One workgroup per output slot of the
// chunk; lag_int is read (the coarse lag0) and all three outputs are overwritten in place.
static int refine_chunk(rmx_ctx* c, const XcorrCall& call, const SpecView& sv, int w0, int wc, int n_pairs, int* d_lag, float* d_frac,
                        float* d_peak, const CafWinner* cw = nullptr) {
    const int rc_p = ensure_ref_pairs(c, n_pairs), logL = sv.logL, unit_log2 = sv.unit_log2;
    if (rc_p != RMX_OK) return rc_p;
    RefineArgs a;
    a.spec = static_cast<const float2*>(sv.base);
    a.pairs = c->rf_pairs;
    a.lb = call.lb;
    a.first_out = w0 / call.integ;
    a.n_buoys = c->n_buoys;
    a.n_pairs = n_pairs;
    a.logL = logL;
    a.row_bits = sv.row_bits;
    a.k = call.integ;
    a.scale = std::ldexp(1.0f, -logL - 2 * unit_log2);   // (1 / L) over the two stored forward scales 2^unit_log2
    // banded call: one slot per VIRTUAL window, rows and lag intervals from virtual window w0 * n_bands on, the spectra per
    // real window; the band set's w0 is the chunk's first real window.  Banded and integrated: one slot per row
    // group * n_bands + band, from row (w0 / K) * n_bands on, the kernel walking the group's real windows
    const int nb = call.banded() ? call.bs.n_bands : 1;
    a.first_out *= nb;
    BandSet bs = call.bs;
    bs.w0 = w0;
    const unsigned grid = (unsigned)(wc / call.integ * nb * n_pairs);
    // k_refine<U, layout>; U was checked by the entry (16 is the last it admits), the four-step layout is the last one
    return with_one_of<kRefKfwd, kRefSmall, kRefRows>(sv.layout, [&](auto lay) {
        return with_one_of<2, 4, 8, 16>(call.refine, [&](auto u) {
            if (cw)   // rmx_caf_batch_quality / _integrated: operand j from the winner's de-rotated set (never banded; a.k windows per slot)
                return launch(c, kTkRefine, k_refine<decltype(u)::value, decltype(lay)::value, CafWinner>, dim3(grid), dim3(kRefThreads), 0,
                              a, d_lag, d_frac, d_peak, *cw);
            if (call.banded() && call.integrated())
                return launch(c, kTkRefine, k_refine<decltype(u)::value, decltype(lay)::value, LagBounds, Integrate, BandSet>, dim3(grid),
                              dim3(kRefThreads), 0, a, d_lag, d_frac, d_peak, call.lb, Integrate{call.integ}, bs);
            if (call.banded())
                return launch(c, kTkRefine, k_refine<decltype(u)::value, decltype(lay)::value, BandSet>, dim3(grid), dim3(kRefThreads), 0, a,
                              d_lag, d_frac, d_peak, bs);
            return launch(c, kTkRefine, k_refine<decltype(u)::value, decltype(lay)::value>, dim3(grid), dim3(kRefThreads), 0, a, d_lag,
                          d_frac, d_peak);
        });
    });
}

// The quality figures of a quality call (quality.hpp) on the chunk the pair kernels have just finished, in front of
// refine_chunk: d_peak still holds the coarse peaks.  One workgroup per output slot of the chunk; nothing but
// call.quality is written.
static int quality_chunk(rmx_ctx* c, const XcorrCall& call, const SpecView& sv, int w0, int wc, int n_pairs, const float* d_peak,
                         const CafWinner* cw = nullptr) {
    const int rc_p = ensure_ref_pairs(c, n_pairs), logL = sv.logL, unit_log2 = sv.unit_log2;
    if (rc_p != RMX_OK) return rc_p;
    QualityArgs a;
    a.spec = static_cast<const float2*>(sv.base);
    a.pairs = c->rf_pairs;
    a.first_out = w0 / call.integ;
    a.n_buoys = c->n_buoys;
    a.n_pairs = n_pairs;
    a.logL = logL;
    a.row_bits = sv.row_bits;
    a.k = call.integ;
    a.sa = std::ldexp(1.0f, -logL - 2 * unit_log2);   // (1 / L) over the stored forward scale 2^unit_log2, squared
    a.sc = std::ldexp(1.0f, -logL - 4 * unit_log2);   // ... to the fourth power
    const int nb = call.banded() ? call.bs.n_bands : 1;   // (banded call: as refine_chunk)
    a.first_out *= nb;
    BandSet bs = call.bs;
    bs.w0 = w0;
    const unsigned grid = (unsigned)(wc / call.integ * nb * n_pairs);
    return with_one_of<kRefKfwd, kRefSmall, kRefRows>(sv.layout, [&](auto lay) {
        if (cw)   // rmx_caf_batch_quality, as refine_chunk
            return launch(c, kTkQuality, k_quality<decltype(lay)::value, CafWinner>, dim3(grid), dim3(kRefThreads), 0, a, d_peak, call.quality,
                          *cw);
        if (call.banded() && call.integrated())
            return launch(c, kTkQuality, k_quality<decltype(lay)::value, LagBounds, Integrate, BandSet>, dim3(grid), dim3(kRefThreads), 0, a,
                          d_peak, call.quality, call.lb, Integrate{call.integ}, bs);
        if (call.banded())
            return launch(c, kTkQuality, k_quality<decltype(lay)::value, BandSet>, dim3(grid), dim3(kRefThreads), 0, a, d_peak, call.quality, bs);
        return launch(c, kTkQuality, k_quality<decltype(lay)::value>, dim3(grid), dim3(kRefThreads), 0, a, d_peak, call.quality);
    });
}

// ---- the selection tables: a run-time length -> the instantiation compiled for it (with_one_of: a length outside a
// list gets the list's last entry; 0 stands for the run-time-length instantiation) -----------------------------------
// column kernels with the column length compiled in (16-column tiles, the default thread count), else the run-time ones
// (LB: empty, or LagBounds / LagBounds, Integrate / LagBounds, Integrate, BandSet for the bounded / integrating / banded
// integrating instantiations of the same set)
template <class... LB>
static auto cols_inv_fn(int l1, int lt, int thr) {
    using namespace gen;
    if (lt == 3) return &g_cols_inv<3, 0, LB...>;
    if (lt == 5)            // 32-column tiles (256-byte row segments): option col_logt = 5, an A/B switch (VERDICT r04 #3a)
        return with_one_of<8, 9, 0>(thr == cols_threads(l1, 5) ? l1 : 0, [](auto L1) { return &g_cols_inv<5, decltype(L1)::value, LB...>; });
    return with_one_of<5, 6, 7, 8, 9, 0>(thr == cols_threads(l1, 4) ? l1 : 0, [](auto L1) { return &g_cols_inv<4, decltype(L1)::value, LB...>; });
}
template <bool U8>
static auto cols_fwd_fn(int l1, int lt, int thr) {
    using namespace gen;
    if (lt == 3) return &g_cols_fwd<U8, 3>;
    if (lt == 5) return with_one_of<8, 9, 0>(thr == cols_threads(l1, 5) ? l1 : 0, [](auto L1) { return &g_cols_fwd<U8, 5, decltype(L1)::value>; });
    return with_one_of<5, 6, 7, 8, 9, 0>(thr == cols_threads(l1, 4) ? l1 : 0, [](auto L1) { return &g_cols_fwd<U8, 4, decltype(L1)::value>; });
}
// row kernels with the row length compiled in where we have it and the threads per row are the default (option rows_tpr)
template <class... WT>   // WT: empty, or XWeight for the weighted instantiations of the same set
static auto rows_fwd_fn(int logR, int tpr) {
    return with_one_of<9, 10, 11, 12, 13, 0>(tpr == gen::rows_tpr(1 << logR) ? logR : 0,
                                             [](auto R) { return &gen::g_rows<true, false, false, decltype(R)::value, WT...>; });
}
template <class... BS>   // BS: empty, or BandSet for the banded instantiations of the same set
static auto rows_inv_fn(int logR, int tpr) {
    return with_one_of<9, 10, 11, 12, 13, 0>(tpr == gen::rows_tpr(1 << logR) ? logR : 0,
                                             [](auto R) { return &gen::g_rows<false, true, true, decltype(R)::value, BS...>; });
}
static decltype(GenericKernels::rows_anchor) rows_anchor_fn(int logR, int tpr) {   // (no run-time-length instantiation: null)
    if (tpr != gen::rows_tpr(1 << logR) || logR < 9 || logR > 13) return nullptr;
    return with_one_of<9, 10, 11, 12, 13>(logR, [](auto R) { return &gen::g_rows_anchor<decltype(R)::value>; });
}
template <bool DEF>
static auto fused_fn(int nb, int logR) {                    // g_rows_fused<n_buoys, log2 row length, default plan>
    return with_one_of<2, 3, 4>(nb, [&](auto NB) {
        return with_one_of<9, 10, 11, 12>(logR, [](auto R) { return &gen::g_rows_fused<decltype(NB)::value, decltype(R)::value, DEF>; });
    });
}
template <bool DEF, bool U8>
static auto wfused_fn(int nb, int logR) {                   // g_win_fused<n_buoys, log2 L, default plan, uint8 input>
    return with_one_of<2, 3, 4>(nb, [&](auto NB) {
        return with_one_of<9, 10, 11, 12>(logR, [](auto R) { return &gen::g_win_fused<decltype(NB)::value, decltype(R)::value, DEF, U8>; });
    });
}
template <bool U8>
static auto wscr_fn(int logR) {                             // g_win_scr<log2 L, uint8 input>
    return with_one_of<9, 10, 11, 12, 13, 14>(logR, [](auto R) { return &gen::g_win_scr<decltype(R)::value, U8>; });
}
static void wscr_shape(int logR, int* thr, int* upw, size_t* lds) {
    with_one_of<9, 10, 11, 12, 13, 14>(logR, [&](auto R) {
        using Plan = gen::WinPlan<decltype(R)::value>;
        *thr = Plan::thr;  *upw = Plan::upw;  *lds = Plan::lds_bytes;
    });
}
// Every kernel choice of the generic path, from the ctx's geometry and the options alone (no HIP call).  g.small: the
// LDS-resident lengths (g_fwd_small / g_pair_small need no choice), else the four-step split L = L1 x L2 with its
// column tile, column threads and threads per row.
static GenericKernels pick_generic_kernels(const gen::Geometry& g, const host::Knobs& knobs) {
    const int n_buoys = g.n_buoys, logL = g.logL, logL1 = g.logL1, logL2 = g.logL2;
    const int col_log_t = g.col_log_t, cols_threads = g.cols_threads, rows_tpr = g.rows_tpr;
    GenericKernels k;
    if (g.small) {
        // at most four buoys, 512 <= L <= 4096: whole windows in one kernel, spectra in registers (option wfused = 0: the
        // two per-transform kernels, as for custom Doppler searches)
        if (n_buoys >= 2 && n_buoys <= 4 && logL >= 9 && logL <= 12 && knobs.get_or("wfused", 1) != 0) {
            k.wf[0][0] = wfused_fn<false, false>(n_buoys, logL);
            k.wf[0][1] = wfused_fn<false, true>(n_buoys, logL);
            k.wf[1][0] = wfused_fn<true, false>(n_buoys, logL);
            k.wf[1][1] = wfused_fn<true, true>(n_buoys, logL);
        }
    } else {
        k.cols_inv = cols_inv_fn<>(logL1, col_log_t, cols_threads);
        k.cols_inv_lb = cols_inv_fn<LagBounds>(logL1, col_log_t, cols_threads);
        k.cols_inv_int = cols_inv_fn<LagBounds, Integrate>(logL1, col_log_t, cols_threads);
        k.cols_inv_int_bs = cols_inv_fn<LagBounds, Integrate, BandSet>(logL1, col_log_t, cols_threads);
        k.cols_fwd[0] = cols_fwd_fn<false>(logL1, col_log_t, cols_threads);
        k.cols_fwd[1] = cols_fwd_fn<true>(logL1, col_log_t, cols_threads);
        k.rows_fwd = rows_fwd_fn<>(logL2, rows_tpr);
        k.rows_fwd_wt = rows_fwd_fn<XWeight>(logL2, rows_tpr);
        k.rows_inv = rows_inv_fn<>(logL2, rows_tpr);
        k.rows_inv_bs = rows_inv_fn<BandSet>(logL2, rows_tpr);
        if (knobs.get_or("rows_anchor", 1) != 0) k.rows_anchor = rows_anchor_fn(logL2, rows_tpr);
        // both row passes in one kernel when the buoys' spectra rows fit the register file (generic_path.hpp); option
        // fused = 0: never, fused_def = 0: without the unrolled default-plan instantiation
        if (n_buoys <= 4 && logL2 >= 9 && logL2 <= 12 && knobs.get_or("fused", 1) != 0) {
            k.fused = fused_fn<false>(n_buoys, logL2);
            if (knobs.get_or("fused_def", 1) != 0) k.fused_def = fused_fn<true>(n_buoys, logL2);
        }
    }
    // any buoy count, 512 <= L <= 16384 (15: the even / odd-bin halves, win_eo.hpp): whole windows in one persistent
    // kernel, spectra in a per-workgroup scratch (option wscr = 0: the two-kernel LDS path / the four-step path, which
    // the Doppler search uses in any case)
    if (!k.wf[0][0] && logL >= 9 && logL <= 15 && knobs.get_or("wscr", 1) != 0) {
        wscr_shape(logL, &k.ws_thr, &k.ws_upw, &k.ws_lds);
        if (logL == 15) {
            k.ws15[0] = gen::g_win_eo15<false>;
            k.ws15[1] = gen::g_win_eo15<true>;
            k.ws_thr = 512;
            k.ws_upw = 1;
            k.ws_lds = gen::Win14Lds::bytes;
        } else if (logL == 14 && knobs.get_or("wscr14", 1) != 0) {
            // L = 16384: 512 threads x two butterflies (g_win_scr14) unless wscr14 = 0 (1024 threads x one: g_win_scr<14>)
            k.ws[0] = gen::g_win_scr14<false>;
            k.ws[1] = gen::g_win_scr14<true>;
            k.ws_thr = 512;
            k.ws_lds = gen::Win14Lds::bytes;
        } else {
            k.ws[0] = wscr_fn<false>(logL);
            k.ws[1] = wscr_fn<true>(logL);
        }
    }
    return k;
}

static int generic_init(rmx_ctx* c) {
    using namespace gen;
    c->generic = true;
    c->geo = make_geometry(c->n_buoys, c->n_samples, c->knobs);
    const Geometry& g = c->geo;
    if (!g.layouts_ok) return fail(c, RMX_E_INVAL, "generic path: an LDS layout of this length and these options overruns its launch bytes");
    const long L = 1L << g.logL;
    std::vector<float2> t;
    int rc = RMX_OK;
    c->gk = pick_generic_kernels(g, c->knobs);
    if (g.small) {
        make_row_table(t, (int)L);
        RMX_MEM(c->g_tw.assign(t));
        rc = allow_lds(c, g.small_allow_lds, g_pair_small<>, g_pair_small<LagBounds>, g_pair_small<LagBounds, Integrate>,
                       g_pair_small<LagBounds, Integrate, CafOperand>, g_pair_small<LagBounds, Integrate, BandSet>, g_pair_small<BandSet>, g_pair_small<LagBounds, BandSet>, g_fwd_small<false>, g_fwd_small<true>,
                       g_fwd_small<false, XWeight>, g_fwd_small<true, XWeight>);
        for (int d = 0; d < 2 && rc == RMX_OK; ++d) rc = allow_lds(c, g.wfused_lds[d], c->gk.wf[d][0], c->gk.wf[d][1]);
        if (rc) return rc;
    } else {
        // the split L = L1 x L2, the column tile and the thread counts: make_geometry (gen_geometry.hpp)
        make_row_table(t, 1 << g.logL1);
        RMX_MEM(c->g_tw1.assign(t));
        make_row_table(t, 1 << g.logL2);
        RMX_MEM(c->g_tw2.assign(t));
        std::vector<float2> thi, tlo;
        make_big_tables(thi, tlo, L, g.lo_bits);
        RMX_MEM(c->g_thi.assign(thi));
        RMX_MEM(c->g_tlo.assign(tlo));
        const GenericKernels& k = c->gk;
        rc = allow_lds(c, g.cols_lds, k.cols_inv, k.cols_inv_lb, k.cols_inv_int, k.cols_inv_int_bs, k.cols_fwd[0], k.cols_fwd[1]);
        // (the run-time-length row kernels too, whichever the tables chose)
        if (rc == RMX_OK)
            rc = allow_lds(c, g.rows_lds, g_rows<true, false, false>, g_rows<false, true, true>, k.rows_fwd, k.rows_fwd_wt, k.rows_inv, k.rows_inv_bs,
                           k.rows_anchor);
        if (rc == RMX_OK) rc = allow_lds(c, g.fused_lds[0], k.fused);
        if (rc == RMX_OK) rc = allow_lds(c, g.fused_lds[1], k.fused_def);
        if (rc) return rc;
        { long v; if (c->knobs.get("rows_anchor", &v) && v >= 2) c->g_rows_anchor_min_b = (int)v; }
        c->g_fused = k.fused != nullptr;
        c->g_fused_always = c->knobs.get_or("fused", 1) == 2;   // 2: also for batches too small to fill the chip (tests)
    }
    c->g_wfused = c->gk.wf[0][0] != nullptr;
    c->g_wscr = c->gk.ws[0] != nullptr || c->gk.ws15[0] != nullptr;
    c->g_wscr_always = c->knobs.get_or("wscr", 1) == 2;         // 2: also for batches that do not fill the chip (tests)
    if (c->g_wscr) {
        const GenericKernels& k = c->gk;
        make_row_table(t, c->geo.logL == 15 ? 16384 : (int)L);       // (N = 16384: two 16384-point halves)
        RMX_MEM(c->g_tw_win.assign(t));
        if (c->geo.logL == 15) {
            const double two_pi = 6.283185307179586476925286766559;
            std::vector<float2> wl(1024);
            for (int i = 0; i < 1024; ++i) wl[i] = make_float2((float)std::cos(two_pi * i / 32768.0), (float)-std::sin(two_pi * i / 32768.0));
            RMX_MEM(c->g_tw_l.assign(wl));
        }
        rc = allow_lds(c, k.ws_lds, k.ws[0], k.ws[1], k.ws15[0], k.ws15[1]);
        if (rc) return rc;
        int per_cu = 1;
        RMX_HIP(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.ws15[0] ? kernel_handle(k.ws15[0]) : kernel_handle(k.ws[0]), k.ws_thr,
                                                                k.ws_lds));
        if (per_cu < 1) per_cu = 1;
        { long v; if (c->knobs.get("wscr_per_cu", &v) && v >= 1 && v <= per_cu) per_cu = (int)v; }
        long grid = (long)c->n_cus * per_cu;
        const long need = ((long)c->max_windows + k.ws_upw - 1) / k.ws_upw;
        if (grid > need) grid = need;
        c->g_ws_grid = (int)grid;
        const size_t sbytes = (size_t)grid * k.ws_upw * c->n_buoys * L * 8;
        RMX_MEM(c->g_ws_scratch.reserve(sbytes / sizeof(float4)));
        // N = 8192: the two bin-parity halves on the fused N = 4096 kernel's network (kwin8k.hpp), same scratch size
        // (B x 2 x 64 KiB per persistent workgroup), one workgroup per CU.  Option kwin8k: 1 (default) = k_win8kl, one anchor
        // half resident in LDS -- 0.51 against g_win_scr14's 0.73 ms at 8 buoys x 512 windows, 1.00 against 1.42 at 16 x 256,
        // 0.19 against 0.285 at 3 x 1024 --; 0 = g_win_scr14; 2 = k_win8k (no resident anchor: -DRMX_EXPERIMENTS builds only)
        if (c->geo.logL == 14 && c->knobs.get_or("kwin8k", 1) != 0) {
            std::vector<float4> t1;
            std::vector<float4> t1_4096;
            std::vector<float2> t2;
            build_tables(t1_4096, t2);
#ifdef RMX_EXPERIMENTS
            if (c->knobs.get_or("kwin8k", 1) == 2) k8::build_tables8k(t1);      // (k_win8k: a full TW1 table per half)
            else
#endif
            k8::build_tables8kl(t1);
            RMX_MEM(c->g_k8_tw1.assign(t1));
            RMX_MEM(c->g_k8_tw2.assign(t2));
            rc = allow_lds(c, k8::kLdsLBytes, k8::k_win8kl<false>, k8::k_win8kl<true>, k8::k_win8kl<false, LagBounds>, k8::k_win8kl<true, LagBounds>);
            if (rc) return rc;
            c->g_k8 = k.ws_upw == 1 && grid <= c->n_cus;      // (its grid is the scratch's: one window slot per workgroup)
            c->g_k8_kind = (int)c->knobs.get_or("kwin8k", 1);
#ifdef RMX_EXPERIMENTS
            rc = allow_lds(c, k8::kLds8Bytes, k8::k_win8k<false>, k8::k_win8k<true>);
            if (rc) return rc;
#else
            if (c->g_k8_kind == 2) return fail(c, RMX_E_UNSUPPORTED, "option kwin8k = 2 (k_win8k) exists only in a -DRMX_EXPERIMENTS build");
#endif
        }
        // N = 16384: four quarter transforms on the same network, forward and pair kernels per chunk of g_ws_grid windows
        // (kwin16k.hpp; the spectra of a chunk take the SAME B x 256 KiB per window as g_win_eo15's per-workgroup scratch, so
        // the buffer is shared).  Option kwin16k: 1 (default) = from the measured batch size on, 2 = every batch, 0 = g_win_eo15.
        if (c->geo.logL == 15 && c->knobs.get_or("kwin16k", 1) != 0 && k.ws_upw == 1) {
            std::vector<float4> t1, t1_4096;
            std::vector<float2> t2, gq, tws;
            build_tables(t1_4096, t2);
            k16::build_tables16k(t1, gq, tws);
            RMX_MEM(c->g_k16_tw1.assign(t1));
            RMX_MEM(c->g_k16_gq.assign(gq));
            RMX_MEM(c->g_k16_tw2.assign(t2));
            RMX_MEM(c->g_k16_tws.assign(tws));
            rc = allow_lds(c, k16::kLdsFwdBytes, k16::k16_fwd<false>, k16::k16_fwd<true>);
            if (rc == RMX_OK) rc = allow_lds(c, k16::kLdsPairBytes, k16::k16_pairs<>, k16::k16_pairs<LagBounds>);
            if (rc) return rc;
            c->g_k16 = (int)c->knobs.get_or("kwin16k", 1);
        }
    }
    // windows per chunk (host_plan.hpp: spectra + products under 32 GiB of the 288, "gen_chunk" caps it for experiments)
    const long chunk = host::generic_chunk_windows(c->n_buoys, L, c->max_windows, 32L << 30, c->knobs.get_or("gen_chunk", 0));
    c->g_chunk = (int)chunk;
    return RMX_OK;
}

// Device buffers of the generic path, allocated on first need:
//   need_spec      the per-window spectra (two-kernel LDS path, four-step path, Doppler search)
//   need_pairbufs  products / tile records / halo of the FOUR-STEP pair kernels -- not when the whole-window kernels
//                  run (g_win_fused, g_win_scr never touch them: an 8-buoy, 4096-window engine of 8192-sample windows
//                  would otherwise pin 15 GB it never uses)
// A failed allocation halves the chunk and retries (down to one window) instead of giving up.
// n_bands > 1 (rmx_xcorr_batch_bands): the pair-dependent buffers hold the slots host::plan_bands states for the chunk.
static int generic_ensure(rmx_ctx* c, int n_pairs, bool need_spec = true, bool need_pairbufs = true, int n_bands = 1) {
    using namespace gen;
    const long L = 1L << c->geo.logL;
    const bool four_step = !c->geo.small;
    auto release = [&]() {   // every chunk-sized buffer
        c->g_spec.release();
        c->g_spec_r.release();
        c->g_prod.release();
        c->g_rec.release();
        c->g_halo.release();
    };
    for (;;) {
        const long parts = c->geo.col_tiles;   // one record per column tile (four-step; else 0)
        const host::BandsPlan bp = host::plan_bands(c->g_chunk, 0, n_bands, c->n_buoys, n_pairs, L, four_step, parts, c->geo.logL1, sizeof(GTile));
        bool ok = !need_spec || c->g_spec.try_reserve((size_t)c->g_chunk * c->n_buoys * L);
        // the pair-dependent buffers grow with the slots (n_bands = 1: g_chunk * n_pairs): each of their sizes is per slot
        if (four_step && need_pairbufs)
            ok = ok && c->g_prod.try_reserve(bp.prod_bytes / sizeof(float2)) && c->g_rec.try_reserve(bp.rec_bytes / sizeof(GTile)) &&
                 c->g_halo.try_reserve(bp.halo_bytes / sizeof(float));
        if (ok) break;
        release();                                    // they come back at half the size
        if (c->g_chunk <= 1) return fail(c, RMX_E_NOMEM, "device allocation failed even for one window per chunk");
        c->g_chunk = (c->g_chunk + 1) / 2;
    }
    if (c->g_pairs.holds(c->plan_pairs)) return RMX_OK;
    std::vector<GPair> gp(n_pairs);
    for (int q = 0; q < n_pairs; ++q) gp[q] = GPair{c->plan_pairs[2 * q], c->plan_pairs[2 * q + 1]};
    RMX_MEM(c->g_pairs.refill(c->plan_pairs, gp));
    return RMX_OK;
}

// forward spectra of windows [w0, w0 + wc) of d_iq into g_spec (rot == nullptr) or, de-rotated by the phasor
// table rot[N], into g_spec_r (rmx_caf_batch); a weighted call weights either (rmx_caf_batch_request)
static int generic_forward(rmx_ctx* c, const XcorrCall& call, const void* d_iq, int w0, int wc, bool u8, const float2* rot,
                           bool cols_only) {
    using namespace gen;
    const int N = c->n_samples, logL = c->geo.logL, B = c->n_buoys;
    const long L = 1L << logL;
    const float fwd_scale = std::ldexp(1.0f, -(logL / 2));
    const int items = wc * B;
    const long first_item = (long)w0 * B;
    if (rot) RMX_MEM(c->g_spec_r.reserve((size_t)c->g_chunk * B * L));   // chunk-sized: generic_ensure releases it with the others
    float2* dst = rot ? c->g_spec_r : c->g_spec;
    XWeight wt = call.wt;   // weighted call: the stored bins carry fwd_scale
    wt.unit = fwd_scale;
    const Geometry& g = c->geo;
    if (g.small) {
        const int sthr = g.small_threads;
        return with_u8(u8, [&](auto U) {
            constexpr bool U8 = decltype(U)::value;
            auto go = [&](auto kern, const float2* a_rot, auto... a_wt) {
                return launch(c, kTkFwdSmall, kern, dim3(items), dim3(sthr), g.small_fwd_lds, d_iq, dst, c->g_tw, N, logL, first_item,
                              fwd_scale, a_rot, a_wt...);
            };
            return call.wt.band ? go(g_fwd_small<U8, XWeight>, rot, wt) : go(g_fwd_small<U8>, rot);
        });
    }
    const int l1 = c->geo.logL1, l2 = c->geo.logL2, L1 = 1 << l1, L2 = 1 << l2;
    const int cthr = g.cols_threads, tpr = g.rows_tpr, ntiles = g.col_tiles;
    // column pass (zero-padded window -> [k1'][n2] * W_L^(n2 k1)), row pass in place (-> [k1'][k2'])
    int rc = launch(c, kTkColsFwd, c->gk.cols_fwd[u8 ? 1 : 0], dim3(ntiles, items), dim3(cthr), g.cols_lds, d_iq, dst, c->g_tw1,
                    l1, l2, first_item, c->geo.lo_bits, c->g_thi, c->g_tlo, rot);
    if (rc != RMX_OK || cols_only) return rc;   // (cols_only: g_rows_fused does the rows)
    const long rows = (long)items * L1;
    const int rpw = kGThreads / tpr;
    // forward rows read no second operand: no spectra, no pair list; a weighted call's chunk starts at window w0
    auto go = [&](auto kern, auto... a_wt) {
        return launch(c, kTkRowsFwd, kern, dim3((unsigned)((rows + rpw - 1) / rpw)), dim3(kGThreads), g.rows_lds, dst, c->g_tw2, l2,
                      L1, l1, L, c->geo.lo_bits, c->g_thi, c->g_tlo, fwd_scale, rows, /* spec */ nullptr, /* spec_j */ nullptr,
                      /* pairs */ nullptr, /* n_pairs */ 0, /* n_buoys */ 0, tpr, a_wt...);
    };
    wt.w0 = w0;
    return call.wt.band ? go(c->gk.rows_fwd_wt, wt) : go(c->gk.rows_fwd);
}

// pair kernels of that chunk: X_i from g_spec, X_j from g_spec (use_rot false) or g_spec_r; results at
// [(w0 + wl) * n_pairs + q] of the three output arrays
static int generic_pairs(rmx_ctx* c, const XcorrCall& call, int w0, int wc, int n_pairs, int* d_lag, float* d_frac, float* d_peak,
                         bool use_rot, bool fused) {
    using namespace gen;
    const int N = c->n_samples, logL = c->geo.logL, B = c->n_buoys;
    const long L = 1L << logL;
    const int hs = logL / 2;
    const float out_scale = std::ldexp(1.0f, -(logL - 2 * hs));
    // banded call: n_bands virtual windows per window, from virtual window v0 on; every slot count below is virtual
    const int nb = call.banded() ? call.bs.n_bands : 1;
    const long v0 = (long)w0 * nb;
    BandSet bs = call.bs;
    bs.w0 = w0;
    const int slots = wc * nb * n_pairs;
    const float2* spec_j = use_rot ? c->g_spec_r : c->g_spec;
    const Geometry& g = c->geo;
    if (g.small) {
        auto go = [&](auto kern, int grid, long first, auto... tail) {
            return launch(c, kTkPairSmall, kern, dim3(grid), dim3(g.small_threads), g.small_pair_lds, c->g_spec, spec_j, c->g_tw,
                          c->g_pairs, n_pairs, B, N, logL, first, out_scale, d_lag, d_frac, d_peak, tail...);
        };
        if (call.integrated() && call.banded())   // one workgroup per (group, band, pair); the bounds per row group * n_bands + band
            return go(g_pair_small<LagBounds, Integrate, BandSet>, slots / call.integ, v0 / call.integ, call.lb, Integrate{call.integ}, bs);
        if (call.integrated() && use_rot)   // rmx_caf_batch_integrated: operand j from the de-rotated set of one hypothesis
            return go(g_pair_small<LagBounds, Integrate, CafOperand>, slots / call.integ, (long)(w0 / call.integ), call.lb,
                      Integrate{call.integ}, CafOperand{0});
        if (call.integrated())   // one workgroup per (group, pair); w0 and wc are whole groups, the bounds per group
            return go(g_pair_small<LagBounds, Integrate>, slots / call.integ, (long)(w0 / call.integ), call.lb, Integrate{call.integ});
        if (call.banded()) return call.bounded() ? go(g_pair_small<LagBounds, BandSet>, slots, v0, call.lb, bs) : go(g_pair_small<BandSet>, slots, v0, bs);
        if (call.bounded()) return go(g_pair_small<LagBounds>, slots, (long)w0, call.lb);
        return go(g_pair_small<>, slots, (long)w0);
    }
    const GenericKernels& k = c->gk;
    const int l1 = c->geo.logL1, l2 = c->geo.logL2, L1 = 1 << l1, L2 = 1 << l2;
    const int cthr = g.cols_threads, tpr = g.rows_tpr, lt = g.col_log_t, ntiles = g.col_tiles;
    const size_t clds = g.cols_lds, rlds = g.rows_lds;
    const long rows = (long)slots * L1;
    const int rpw = kGThreads / tpr;
    const bool all_pairs = c->plan_all_pairs && n_pairs == B * (B - 1) / 2;
    // row pass ([product on load] rows(L2)^-1 * conj W_L^(n2 k1)), column pass (-> tile records + halo), reduction
    int rc;
    if (call.banded()) {
        // always the product-on-load rows: their banded instantiation masks the product (never g_rows_anchor / g_rows_fused)
        rc = launch(c, kTkRowsInv, k.rows_inv_bs, dim3((unsigned)((rows + rpw - 1) / rpw)), dim3(kGThreads), rlds, c->g_prod, c->g_tw2, l2, L1,
                    l1, L, c->geo.lo_bits, c->g_thi, c->g_tlo, 1.0f, rows, c->g_spec, spec_j, c->g_pairs, n_pairs, B, tpr, bs);
    } else if (fused) {
        // g_spec holds the column pass's output: forward rows, products and inverse rows in one kernel
        const long units = (long)wc * L1;
        const int upw = kGThreads / (L2 >> 4 > 0 ? L2 >> 4 : 1);
        const bool def_plan = k.fused_def && all_pairs;
        const float fs = std::ldexp(1.0f, -(logL / 2));
        rc = launch(c, kTkRowsFused, def_plan ? k.fused_def : k.fused, dim3((unsigned)((units + upw - 1) / upw)), dim3(kGThreads),
                    g.fused_lds[def_plan ? 1 : 0], c->g_spec, c->g_prod, c->g_tw2, L1, l1, L, c->geo.lo_bits,
                    c->g_thi, c->g_tlo, fs * fs, units, c->g_pairs, n_pairs);
    } else if (k.rows_anchor && all_pairs && B >= c->g_rows_anchor_min_b) {
        // default pair list: the anchor's row stays in registers over its run of pairs (from 6 buoys on: with 5 the runs are
        // too short for the per-workgroup set-up, 0.649 -> 0.692 ms at N = 16384; with 6 / 7 / 8 buoys 0.89 -> 0.84, 1.16 -> 1.10,
        // 1.54 -> 1.39 ms, cfg5 250 -> 203 ms)
        rc = launch(c, kTkRowsAnchor, k.rows_anchor, dim3((unsigned)((L1 / rpw) * (B - 1)), (unsigned)wc), dim3(kGThreads), rlds, c->g_prod,
                    c->g_tw2, L1, l1, L, c->geo.lo_bits, c->g_thi, c->g_tlo, 1.0f, c->g_spec, spec_j, n_pairs, B);
    } else {
        rc = launch(c, kTkRowsInv, k.rows_inv, dim3((unsigned)((rows + rpw - 1) / rpw)), dim3(kGThreads), rlds, c->g_prod, c->g_tw2, l2, L1,
                    l1, L, c->geo.lo_bits, c->g_thi, c->g_tlo, 1.0f, rows, c->g_spec, spec_j, c->g_pairs, n_pairs, B, tpr);
    }
    if (rc != RMX_OK) return rc;
    // integrated call: the column pass sums the |r|^2 of a group's K product slots tile by tile and leaves one tile record
    // and halo per (group, pair) slot; g_final then reduces those slots as it reduces a window's (the bounds are per group:
    // slot -> group w0 / K + slot / P).  Otherwise K = 1: slot -> window w0 + slot / P, pair slot % P.  Banded and integrated:
    // the banded rows above left one product per virtual window, and the column pass sums the K products of (group, band)
    // where they lie, n_bands * P slots apart; a slot is then (row w0 / K * n_bands + slot / P, pair).
    const int oslots = (int)host::cols_inv_grid_rows(wc, nb, n_pairs, call.integ);   // the planner's count: it cut the chunk by it
    LagBounds lb = call.lb;
    lb.w0 = v0 / call.integ;   // (banded: the bounds are per virtual window; w0 is a multiple of K)
    lb.n_pairs = n_pairs;
    auto cols = [&](auto kern, auto... tail) {
        return launch(c, kTkColsInv, kern, dim3(ntiles, oslots), dim3(cthr), clds, c->g_prod, c->g_tw1, l1, l2, c->g_rec, c->g_halo, tail...);
    };
    rc = call.integrated() && call.banded() ? cols(k.cols_inv_int_bs, lb, Integrate{call.integ}, bs)
         : call.integrated()                ? cols(k.cols_inv_int, lb, Integrate{call.integ})
         : call.bounded()                   ? cols(k.cols_inv_lb, lb)
                                            : cols(k.cols_inv);
    if (rc != RMX_OK) return rc;
    auto reduce = [&](auto kern, auto... tail) {
        return launch(c, kTkFinal, kern, dim3(oslots), dim3(64), 0, N, l1, l2, lt, c->g_rec, c->g_halo, ntiles, oslots, lb.w0 * n_pairs,
                      out_scale, d_lag, d_frac, d_peak, tail...);
    };
    return call.bounded() ? reduce(g_final<LagBounds>, lb) : reduce(g_final<>);   // (an integrated call always carries bounds)
}

// N = 4096, unfused path: forward spectra of windows [w0, w0 + wc) into d_spec (rot == nullptr) or, de-rotated by
// the phasor table rot[N], into d_spec_r (rmx_caf_batch), weighted where the call says so; then the pair kernels over the plan's pair list
static int fwd4096(rmx_ctx* c, const XcorrCall& call, const void* d_iq, int w0, int wc, bool u8, const float2* rot, int n_bins = 1) {
    const long first_item = (long)w0 * c->n_buoys;
    const int wrap = n_bins > 1 ? wc * c->n_buoys : 0;
    const int n_items = wc * c->n_buoys * n_bins;
    if (rot) {
        const size_t nb = n_bins > 1 ? (size_t)n_items * (8 * kThreads) * sizeof(float4)
                                     : (size_t)(wc < c->chunk_windows ? c->chunk_windows : wc) * c->n_buoys * (8 * kThreads) * sizeof(float4);
        RMX_MEM(c->d_spec_r.reserve(nb / sizeof(float4)));
    }
    float4* dst = rot ? c->d_spec_r.get() : c->d_spec.get();
    return with_u8(u8, [&](auto U) {
        constexpr bool U8 = decltype(U)::value;
        auto go = [&](auto kern, const float2* a_rot, int a_wrap, auto... wt) {
            return launch(c, kTkFwd4096, kern, dim3(n_items), dim3(kThreads), kLdsBytes, d_iq, dst, c->d_tw1, c->d_tw2, first_item, 1.0f, a_rot,
                          a_wrap, wt...);
        };
        if (!call.wt.band) return go(k_fwd<U8>, rot, wrap);
        XWeight wt = call.wt;   // weighted call: the stored bins carry the TW1 scale; the band is the real window's under wrap
        wt.unit = (float)kTw1Scale;
        return go(k_fwd<U8, XWeight>, rot, wrap, wt);
    });
}
static int pairs4096(rmx_ctx* c, const XcorrCall& call, int w0, int wc, int n_pairs, int* d_lag, float* d_frac, float* d_peak, float out_scale,
                     bool use_rot, int n_bins = 1) {
    const int n_parts = c->plan_n_parts;
    const int nb = call.banded() ? call.bs.n_bands : 1;   // (banded call: virtual window = window * n_bands + band)
    // all hypotheses in one launch: virtual window = hypothesis * wc + window; banded (rmx_caf_batch_bands): that times
    // n_bands, plus the band, and the wrap counts virtual windows
    const int i_wrap = n_bins > 1 ? wc * nb : 0;
    const long first = (long)w0 * nb;
    wc *= n_bins * nb;
    const int xcd_map = (wc % 8 == 0) ? 1 : 0;
    const float4* spec_j = use_rot ? c->d_spec_r.get() : c->d_spec.get();
    // the streaming and the resident kernel (which keeps one unused int argument), each with or without its trailing structs
    auto str = [&](auto kern, int windows, int xmap, long first, int wrap, auto... tail) {
        return launch(c, kTkPair4096, kern, dim3(windows * n_parts), dim3(kThreads), kLdsBytes, c->d_spec, spec_j, c->d_tw1, c->d_tw2,
                      c->d_items, c->d_part_begin, n_parts, c->n_buoys, n_pairs, xmap, first, out_scale, d_lag, d_frac, d_peak, wrap, tail...);
    };
    auto res = [&](auto kern, auto... lb) {
        return launch(c, kTkPair4096, kern, dim3(wc * n_parts), dim3(kThreads), kLdsResBytes, c->d_spec, spec_j, c->d_tw1, c->d_tw2,
                      c->d_items, c->d_part_begin, n_parts, c->n_buoys, n_pairs, xcd_map, first, out_scale, d_lag, d_frac, d_peak, 0, i_wrap,
                      lb...);
    };
    if (call.integrated() && call.banded()) {
        // the banded integrating instantiation: one work item per (group, band, pair), rows group-major from
        // (w0 / K) * n_bands on (wc counts the chunk's virtual windows here: whole groups times n_bands)
        const int rows = wc / call.integ;
        BandSet bs = call.bs;
        bs.w0 = w0;
        return str(k_pair_str<LagBounds, Integrate, BandSet>, rows, (rows % 8 == 0) ? 1 : 0, first / call.integ, 0, call.lb,
                   Integrate{call.integ}, bs);
    }
    if (call.integrated() && use_rot) {
        // rmx_caf_batch_integrated: operand j from the de-rotated set.  One hypothesis (n_bins == 1): the chunk's groups, as
        // below.  All hypotheses in one launch: virtual group = hypothesis * groups + group (wc counts virtual windows here),
        // operand i and the bounds at the real group, the output slot virtual
        const int gc = wc / call.integ;
        return str(k_pair_str<LagBounds, Integrate, CafOperand>, gc, (gc % 8 == 0) ? 1 : 0, (long)(w0 / call.integ), 0, call.lb,
                   Integrate{call.integ}, CafOperand{i_wrap / call.integ});
    }
    if (call.integrated()) {
        // always the streaming kernel's integrating instantiation, one work item per (group, pair); w0 and wc are whole
        // groups, the bounds per group
        const int gc = wc / call.integ;
        return str(k_pair_str<LagBounds, Integrate>, gc, (gc % 8 == 0) ? 1 : 0, (long)(w0 / call.integ), 0, call.lb, Integrate{call.integ});
    }
    if (call.banded()) {   // the banded instantiations: both spectra of a virtual window are its real window's
        BandSet bs = call.bs;
        bs.w0 = w0;
        if (c->resident) return call.bounded() ? res(k_pair_res<LagBounds, BandSet>, call.lb, bs) : res(k_pair_res<BandSet>, bs);
        return call.bounded() ? str(k_pair_str<LagBounds, BandSet>, wc, xcd_map, first, i_wrap, call.lb, bs)
                              : str(k_pair_str<BandSet>, wc, xcd_map, first, i_wrap, bs);
    }
    if (c->resident) return call.bounded() ? res(k_pair_res<LagBounds>, call.lb) : res(k_pair_res<>);
    return call.bounded() ? str(k_pair_str<LagBounds>, wc, xcd_map, (long)w0, i_wrap, call.lb) : str(k_pair_str<>, wc, xcd_map, (long)w0, i_wrap);
}
static_assert(kL == 1 << 13, "spec_view and out_scale4096 say log2 kL = 13");
static float out_scale4096() {
    // power-of-two scaling: the TW1 table carries 2^-6, so the spectra carry 2^-6, the product 2^-12 and
    // the inverse transform (which uses the table once more) 2^-18; the taps get the remaining factor
    return std::ldexp(1.0f, 3 * kTw1ScaleLog2 - 13);
}

static SpecView spec_view(const rmx_ctx* c) {
    if (!c->generic)   // (the forward scale 2^-6 rides on the TW1 table)
        return {kRefKfwd, c->d_spec, 13 /* log2 kL */, 0, -kTw1ScaleLog2,
                [](rmx_ctx* c, const XcorrCall& call, const void* d_iq, int w0, int wc, bool u8, const float2* rot, bool) {
                    return fwd4096(c, call, d_iq, w0, wc, u8, rot);
                },
                [](rmx_ctx* c, const XcorrCall& call, int w0, int wc, int n_pairs, int* d_lag, float* d_frac, float* d_peak, bool use_rot, bool) {
                    return pairs4096(c, call, w0, wc, n_pairs, d_lag, d_frac, d_peak, out_scale4096(), use_rot);
                }};
    const bool small_l = c->geo.small;
    return {small_l ? kRefSmall : kRefRows, c->g_spec, c->geo.logL, small_l ? 0 : c->geo.logL1, -(c->geo.logL / 2), generic_forward, generic_pairs};
}

// what the planner (host_plan.hpp: plan_route) needs to know of this ctx
static_assert(gen::kGThreads == 256, "host::route_rows_fused counts g_rows_fused's units per workgroup of 256 threads");
static host::RouteCaps route_caps(const rmx_ctx* c) {
    host::RouteCaps k;
    k.n_cus = c->n_cus;  k.n_buoys = c->n_buoys;  k.generic = c->generic;
    k.fused = c->fused;  k.small_batch = c->small_batch;  k.chunk_windows = c->chunk_windows;
    k.ppb_user = c->ppb_user ? c->pairs_per_block : 0;
    if (!c->generic) return k;
    k.logL = c->geo.logL;  k.logL1 = c->geo.logL1;  k.logL2 = c->geo.logL2;  k.small_maxl = c->geo.small_maxl;
    k.g_chunk = c->g_chunk;  k.wfused = c->g_wfused;  k.wscr = c->g_wscr;  k.wscr_always = c->g_wscr_always;
    k.ws_upw = c->gk.ws_upw;  k.ws_grid = c->g_ws_grid;  k.k8 = c->g_k8;  k.k16 = c->g_k16;
    if (c->g_k16 == 1) k.k16_min_windows = c->knobs.get_or("k16_min_windows", 0);
    k.g_fused = c->g_fused;  k.g_fused_always = c->g_fused_always;
    k.max_pairs8 = k8::kMaxPairs8;  k.max_pairs16 = k16::kMaxPairs16;  k.integ_max_per_thread = kIntegMaxPerThread;
    if (!c->geo.small) { k.col_tile = c->geo.col_tile;  k.cols_threads = c->geo.cols_threads; }   // (read for the four-step route only)
    return k;
}

// Windows [w_first, w_first + n) through the per-transform kernels, `chunk` windows at a time (the buffers are there): the
// forward spectra, the pair kernels (with_pairs false: quality_pass, whose lags are there already), then k_quality on the
// spectra and the coarse peaks, then k_refine, which overwrites them.  A qualified or refined call is weighted(): its
// chunks never take g_rows_fused, so the view holds every spectrum of the chunk.
static int run_chunks(rmx_ctx* c, const XcorrCall& call, const host::RouteCaps& caps, const void* d_iq, int w_first, int n, int chunk,
                      int n_pairs, int* d_lag, float* d_frac, float* d_peak, bool u8, bool with_pairs = true) {
    const SpecView sv = spec_view(c);
    for (int w0 = w_first; w0 < w_first + n; w0 += chunk) {
        const int wc = w_first + n - w0 < chunk ? w_first + n - w0 : chunk;
        const bool rows_fused = with_pairs && host::route_rows_fused(caps, call.weighted(), wc);
        int rc = sv.forward(c, call, d_iq, w0, wc, u8, nullptr, rows_fused);
        if (rc == RMX_OK && with_pairs) rc = sv.pairs(c, call, w0, wc, n_pairs, d_lag, d_frac, d_peak, false, rows_fused);
        if (rc == RMX_OK && call.qualified()) rc = quality_chunk(c, call, sv, w0, wc, n_pairs, d_peak);
        if (rc == RMX_OK && call.refined()) rc = refine_chunk(c, call, sv, w0, wc, n_pairs, d_lag, d_frac, d_peak);
        if (rc != RMX_OK) return rc;
    }
    return RMX_OK;
}

// N = 16384 through k16_fwd / k16_pairs (kwin16k.hpp): per chunk of g_ws_grid windows (the spectrum scratch holds that many)
// one forward launch -- (window, buoy) items over at most one workgroup per CU -- and one pair launch of 8 S workgroups,
// S = workgroups per XCD.  No per-window state survives the chunk.
static int k16_batch(rmx_ctx* c, const XcorrCall& call, const void* d_iq, int n_windows, int chunk, int n_pairs, int* d_lag, float* d_frac,
                     float* d_peak, bool u8) {
    const int B = c->n_buoys;
    const float out_scale = std::ldexp(1.0f, 3 * kTw1ScaleLog2 - 15);
    const k16::Pair2* prs = reinterpret_cast<const k16::Pair2*>(c->g_pairs.get());
    for (int w0 = 0; w0 < n_windows; w0 += chunk) {
        const int wc = n_windows - w0 < chunk ? n_windows - w0 : chunk;
        const int items = wc * B;
        const unsigned fgrid = (unsigned)(items < c->n_cus ? items : c->n_cus);
        int rc = with_u8(u8, [&](auto U) {
            return launch(c, kTkFwd16k, k16::k16_fwd<decltype(U)::value>, dim3(fgrid), dim3(kThreads), k16::kLdsFwdBytes, d_iq, c->g_ws_scratch,
                          c->g_k16_tw1, c->g_k16_gq, c->g_k16_tw2, c->g_k16_tws, (long)w0 * B, items);
        });
        if (rc != RMX_OK) return rc;
        // XCD-aware item order (the pairs of a window on one XCD) unless the windows do not spread evenly over eight XCDs
        // and are few: 9 windows would give XCD 0 two windows' work and leave the batch waiting for it
        const int flat = (wc < 32 && wc % 8 != 0) || c->n_cus < 8 ? 1 : 0;
        const long per_xcd = (long)((wc + 7) / 8) * n_pairs;       // items of the busiest XCD
        long S = c->n_cus / 8 > 0 ? c->n_cus / 8 : 1;
        if (per_xcd < S) S = per_xcd;
        long pgrid = 8 * S;
        if (flat) pgrid = (long)wc * n_pairs < c->n_cus ? (long)wc * n_pairs : c->n_cus;
        auto pairs = [&](auto kern, auto... lb) {
            return launch(c, kTkPairs16k, kern, dim3((unsigned)pgrid), dim3(kThreads), k16::kLdsPairBytes, c->g_ws_scratch, c->g_k16_tw1,
                          c->g_k16_gq, c->g_k16_tw2, c->g_k16_tws, B, prs, n_pairs, (long)w0 * n_pairs, wc, flat, out_scale, d_lag, d_frac,
                          d_peak, lb...);
        };
        if (call.bounded()) {   // the same kernel with the lag windows (lb.w0: window 0 of this launch)
            LagBounds lb = call.lb;
            lb.w0 = w0;
            lb.n_pairs = n_pairs;
            rc = pairs(k16::k16_pairs<LagBounds>, lb);
        } else
            rc = pairs(k16::k16_pairs<>);
        if (rc != RMX_OK) return rc;
    }
    return RMX_OK;
}

// a refusal of the planner as the caller reads it
static int route_refusal(rmx_ctx* c, host::RouteRefusal refused, int bands_chunk, const host::RouteCaps& k, int integ, int n_bands,
                         int n_pairs = 0) {
    if (refused == host::kRouteOk) return RMX_OK;
    if (refused == host::kRefuseBandsChunk)
        return fail(c, RMX_E_INVAL, "n_bands = %d bands x %d pairs are more slots per window than any chunk of this ctx holds (at most %ld, "
                    "their products under %ld bytes): a window's bands are never split", n_bands, n_pairs, host::kMaxGridY,
                    host::kGenericBudgetBytes);
    if (refused == host::kRefuseIntegChunk && bands_chunk > 0)
        return fail(c, RMX_E_INVAL, "integrate = %d windows per group is more than the chunk of %d windows that n_bands = %d bands shrank this "
                    "ctx's chunk of %d windows to: a group is never split", integ, bands_chunk, n_bands, k.g_chunk);
    if (refused == host::kRefuseIntegChunk)
        return fail(c, RMX_E_INVAL, "integrate = %d windows per group is more than the largest chunk this ctx can hold, %d windows",
                    integ, k.generic ? k.g_chunk : k.chunk_windows);
    return fail(c, RMX_E_UNSUPPORTED, "integrated call: a column tile of %ld elements on %d threads is more than %d per thread",
                k.col_tile, k.cols_threads, k.integ_max_per_thread);
}

// The generic lengths: executes the route that host::plan_route chose for the call `rq` describes (host_plan.hpp has the
// rules and the measurements behind them).
static int generic_batch(rmx_ctx* c, const XcorrCall& call, host::RouteCaps caps, const host::RouteCall& rq, host::RoutePlan plan,
                         const void* d_iq, int* d_lag, float* d_frac, float* d_peak, bool u8) {
    using namespace host;
    const GenericKernels& k = c->gk;
    const int n_pairs = rq.n_pairs, logL = c->geo.logL, hs = logL / 2;
    // device buffers on first need; a failed allocation halves g_chunk, and the plan follows (the route does not depend on it)
    auto ensure = [&](bool need_spec, bool need_pairbufs) -> int {
        const int rc_e = generic_ensure(c, n_pairs, need_spec, need_pairbufs, rq.n_bands);
        if (rc_e == RMX_OK && c->g_chunk != caps.g_chunk) { caps.g_chunk = c->g_chunk; plan = plan_route(caps, rq); }
        return rc_e;
    };
    // the whole-window kernels and k16 keep no per-window state in HBM
    const bool per_transform = plan.route == kRouteSmallL || plan.route == kRouteFourStep;
    int rc = ensure(per_transform, per_transform);
    if (rc == RMX_OK) rc = route_refusal(c, plan.refused, plan.bands_chunk, caps, call.integ, rq.n_bands);
    if (rc != RMX_OK) return rc;
    if (per_transform) return run_chunks(c, call, caps, d_iq, 0, rq.n_windows, plan.chunk, n_pairs, d_lag, d_frac, d_peak, u8);
    if (plan.route == kRouteK16) return k16_batch(c, call, d_iq, rq.n_windows, plan.chunk, n_pairs, d_lag, d_frac, d_peak, u8);
    const long n_head = plan.n_head;
    const float fwd_scale = std::ldexp(1.0f, -hs), out_scale = std::ldexp(1.0f, -(logL - 2 * hs));
    if (plan.route == kRouteWinFused) {
        const int upw = gen::kGThreads / ((1 << logL) >> 4), def = rq.all_pairs ? 1 : 0;
        return launch(c, kTkWindow, k.wf[def][u8 ? 1 : 0], dim3((unsigned)((rq.n_windows + upw - 1) / upw)), dim3(gen::kGThreads), c->geo.wfused_lds[def],
                      d_iq, c->g_tw, n_head, 0L, fwd_scale, out_scale, c->g_pairs, n_pairs, d_lag, d_frac, d_peak);
    }
    // g_win_scr*, g_win_eo15, k_win8kl: persistent workgroups over the ctx's scratch; the full rounds here, the planned
    // partial round behind them through the per-transform kernels on the same stream
    long grid = ((long)rq.n_windows + k.ws_upw - 1) / k.ws_upw;
    if (grid > c->g_ws_grid) grid = c->g_ws_grid;
    if (plan.route == kRouteKWin8) {            // N = 8192 on k_win's network (kwin8k.hpp)
        const float out_scale8 = std::ldexp(1.0f, 3 * kTw1ScaleLog2 - 14);
        const k8::Pair2* prs = rq.all_pairs ? nullptr : reinterpret_cast<const k8::Pair2*>(c->g_pairs.get());
        const int stag = (int)c->knobs.get_or("stag", 1);
        rc = with_u8(u8, [&](auto U) {
            constexpr bool U8 = decltype(U)::value;
            auto go = [&](auto kern, size_t lds, auto... lb) {
                return launch(c, kTkWindow, kern, dim3((unsigned)grid), dim3(kThreads), lds, d_iq, c->g_ws_scratch, c->g_k8_tw1, c->g_k8_tw2,
                              c->n_buoys, prs, n_pairs, 0L, out_scale8, d_lag, d_frac, d_peak, plan.n_head, stag, lb...);
            };
#ifdef RMX_EXPERIMENTS
            if (c->g_k8_kind == 2) return go(k8::k_win8k<U8>, k8::kLds8Bytes);
#endif
            return call.bounded() ? go(k8::k_win8kl<U8, LagBounds>, k8::kLdsLBytes, call.lb) : go(k8::k_win8kl<U8>, k8::kLdsLBytes);
        });
    } else if (plan.route == kRouteWinEo15) {   // (g_win_eo15: one more table)
        rc = launch(c, kTkWindow, k.ws15[u8 ? 1 : 0], dim3((unsigned)grid), dim3(k.ws_thr), k.ws_lds, d_iq, c->g_ws_scratch, c->g_tw_win,
                    c->g_tw_l, c->n_buoys, n_head, 0L, fwd_scale, out_scale, c->g_pairs, n_pairs, d_lag, d_frac, d_peak);
    } else {
        rc = launch(c, kTkWindow, k.ws[u8 ? 1 : 0], dim3((unsigned)grid), dim3(k.ws_thr), k.ws_lds, d_iq, c->g_ws_scratch, c->g_tw_win,
                    c->n_buoys, n_head, 0L, fwd_scale, out_scale, c->g_pairs, n_pairs, d_lag, d_frac, d_peak);
    }
    if (rc != RMX_OK || !plan.n_tail) return rc;
    rc = ensure(true, true);
    return rc != RMX_OK ? rc : run_chunks(c, call, caps, d_iq, plan.n_head, plan.n_tail, plan.chunk, n_pairs, d_lag, d_frac, d_peak, u8);
}

}  // namespace rmx

using namespace rmx;

using host::kHostSubChunk;

extern "C" {

int rmx_version(void) { return RMX_VERSION; }

int rmx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char* rmx_last_error(const rmx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int rmx_create(rmx_ctx** out, int device_id, int n_buoys, int n_samples, int max_windows, unsigned flags) {
    if (!out) return fail(nullptr, RMX_E_INVAL, "out is NULL");
    *out = nullptr;
    (void)flags;
    {
        std::string why;
        if (host::check_create_args(n_buoys, n_samples, max_windows, &why) != 0) return fail(nullptr, RMX_E_INVAL, "%s", why.c_str());
    }
    int ndev = rmx_device_count();
    if (ndev <= 0) return fail(nullptr, RMX_E_NODEV, "no HIP device visible");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, RMX_E_INVAL, "device_id %d not in 0..%d", device_id, ndev - 1);
    rmx_ctx* c = new (std::nothrow) rmx_ctx();
    if (!c) return fail(nullptr, RMX_E_NOMEM, "host allocation failed");
    c->knobs = host::snapshot_default_options();   // options set later do not reach this ctx
    c->device = device_id;
    c->n_buoys = n_buoys;
    c->n_samples = n_samples;
    c->max_windows = max_windows;
    int rc = RMX_OK;
    auto bail = [&](int code) {
        g_create_error = c->err;
        rmx_destroy(c);
        return code;
    };
    auto init = [&]() -> int {
        RMX_HIP(c, hipSetDevice(device_id));
        {
            int ncu = 0;
            if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && ncu > 0)
                c->n_cus = ncu;
            // experiment knob: fewer persistent workgroups than CUs (per-CU time without chip-wide contention)
            { long v; if (c->knobs.get("ncus", &v) && v > 0 && v < c->n_cus) c->n_cus = (int)v; }
        }
        RMX_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
        // (option generic4096 = 1: N = 4096 through the generic kernels too -- g_win_scr<13> against k_win, an experiment)
        if (n_samples != kM || c->knobs.get_or("generic4096", 0) != 0) return rmx::generic_init(c);
        int chunk = (int)c->knobs.get_or("chunk_windows", 4096);
        if (chunk < 8) chunk = 8;
        chunk = (chunk + 7) & ~7;
        if (chunk > max_windows) chunk = max_windows;
        {   // spectra scratch = chunk * B * 64 KiB: keep it under 8 GiB
            const long per_win = (long)n_buoys * (8 * kThreads) * (long)sizeof(float4);
            const long cap = (8L << 30) / per_win;
            if (chunk > cap) chunk = (int)(cap > 8 ? (cap & ~7L) : 8);
        }
        c->chunk_windows = chunk;
        // the fused kernel keeps its spectra per persistent workgroup (n_cus * B * 64 KiB); the
        // per-window scratch of the unfused path (custom pair lists) is allocated on first use
        {
            const int wg = chunk < c->n_cus ? chunk : c->n_cus;
            RMX_MEM(c->d_spec.reserve((size_t)wg * n_buoys * (8 * kThreads)));
        }
        std::vector<float4> tw1;
        std::vector<float2> tw2;
        build_tables(tw1, tw2);
        RMX_MEM(c->d_tw1.assign(tw1));
        RMX_MEM(c->d_tw2.assign(tw2));
        const std::vector<int32_t> trail = host::encode_pair_trail(host::plan_pair_trail(n_buoys));
        if (trail.empty()) return fail(c, RMX_E_INVAL, "k_win cannot walk the pair order planned for %d buoys", n_buoys);
        RMX_MEM(c->d_trail.assign(trail));
        c->stag = (int)c->knobs.get_or("stag", 1);
        c->stag_kwin = (int)c->knobs.get_or("stag", 0);
        c->small_batch = c->knobs.get_or("small4096", 1) != 0;
#ifdef RMX_EXPERIMENTS
        {   // the two other builds of the fused kernel: measured slower, not in the default build
            std::vector<float4> t1;
            std::vector<float2> tb, tc;
            build_tables8(t1, tb, tc);
            RMX_MEM(c->d_tw1_8.assign(t1));
            RMX_MEM(c->d_tb8.assign(tb));
            RMX_MEM(c->d_tc8.assign(tc));
            int rc_x = allow_lds(c, w8::kLdsWin8Bytes, w8::k_win8<false>, w8::k_win8<true>);
            if (rc_x == RMX_OK) rc_x = allow_lds(c, pk::kLdsWinpBytes, k_winp<false>, k_winp<true>);
            if (rc_x != RMX_OK) return rc_x;
            c->pk = (int)c->knobs.get_or("pk", 0);
            c->win8 = (int)c->knobs.get_or("win8", 0);
        }
#endif
        // every instantiation of the N = 4096 kernels: plain, weighted (rmx_xcorr_batch_weighted: k_fwd) and bounded
        // (rmx_xcorr_batch_bounded: the peak-searching ones)
        int rc_l = allow_lds(c, kLdsBytes, k_fwd<false>, k_fwd<true>, k_fwd<false, XWeight>, k_fwd<true, XWeight>, k_pair_str<>,
                             k_pair_str<LagBounds>, k_pair_str<BandSet>, k_pair_str<LagBounds, BandSet>,
                             k_pair_str<LagBounds, Integrate, BandSet>, k_pair_str<LagBounds, Integrate, CafOperand>);
        if (rc_l == RMX_OK)
            rc_l = allow_lds(c, kLdsResBytes, k_pair_res<>, k_pair_res<LagBounds>, k_pair_res<BandSet>, k_pair_res<LagBounds, BandSet>);
        if (rc_l == RMX_OK) rc_l = allow_lds(c, kLdsWinBytes, k_win<false>, k_win<true>, k_win_lb<false>, k_win_lb<true>);
        return rc_l;
    };
    rc = init();
    if (rc != RMX_OK) return bail(rc);
    *out = c;
    return RMX_OK;
}

void rmx_destroy(rmx_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->copy_ev)
        if (e) (void)hipEventDestroy(e);
    for (DevStage* s : {&c->lb_stage, &c->band_stage})
        if (s->ev) (void)hipEventDestroy(s->ev);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;   // every buffer frees itself (dev_buf.hpp); nothing of this ctx runs any more
}

int rmx_set_stream(rmx_ctx* c, void* hip_stream) {
    if (!c) return RMX_E_INVAL;
    RMX_HIP(c, hipSetDevice(c->device));
    if (c->stream) RMX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    c->stream = (hipStream_t)hip_stream;
    c->own_stream = false;
    return RMX_OK;
}

int rmx_set_default_option(const char* key, long value) {
    std::string why;
    if (host::set_default_option(key, value, &why) != 0) return fail(nullptr, RMX_E_INVAL, "%s", why.c_str());
    return RMX_OK;
}

void rmx_clear_default_options(void) { host::clear_default_options(); }

int rmx_set_option(rmx_ctx* c, const char* key, long value) {
    if (!c || !key) return RMX_E_INVAL;
    if (!strcmp(key, "chunk_windows")) {
        if (c->generic) return RMX_OK;   // the generic path sizes its own chunks
        long chunk = value < 8 ? 8 : value;
        chunk = (chunk + 7) & ~7L;
        if (chunk > c->max_windows) chunk = c->max_windows;
        {   // same 8 GiB cap on the unfused path's scratch as at creation
            const long per_win = (long)c->n_buoys * (8 * kThreads) * (long)sizeof(float4);
            const long cap = (8L << 30) / per_win;
            if (chunk > cap) chunk = cap > 8 ? (cap & ~7L) : 8;
        }
        c->chunk_windows = (int)chunk;   // (scratch follows on the next call: ensure_spec)
        return RMX_OK;
    }
    if (!strcmp(key, "pairs_per_block")) {
        if (value < 1 || value > 1 << 20) return fail(c, RMX_E_INVAL, "pairs_per_block %ld out of range", value);
        c->pairs_per_block = (int)value;
        c->ppb_user = true;
        return RMX_OK;
    }
    if (!strcmp(key, "dbg")) {
        return fail(c, RMX_E_UNSUPPORTED, "option 'dbg': the timing-only ablation build was removed");
    }
    if (!strcmp(key, "pk") || !strcmp(key, "win8")) {
#ifdef RMX_EXPERIMENTS
        (key[0] == 'p' ? c->pk : c->win8) = value != 0;
        return RMX_OK;
#else
        return fail(c, RMX_E_UNSUPPORTED, "option '%s' exists only in the -DRMX_EXPERIMENTS build (k_win8 / k_winp)", key);
#endif
    }
    if (!strcmp(key, "stag")) {
        if (value < 0 || value > 5) return fail(c, RMX_E_INVAL, "stag %ld not in 0..5", value);
        c->stag = c->stag_kwin = (int)value;
        return RMX_OK;
    }
    if (!strcmp(key, "small4096")) {
        c->small_batch = value != 0;
        return RMX_OK;
    }
    if (!strcmp(key, "fused")) {
        c->fused = value != 0;
        return RMX_OK;
    }
    if (!strcmp(key, "resident")) {
        c->resident = value != 0;
        return RMX_OK;
    }
    if (!strcmp(key, "timing")) {
        c->timing = value != 0;
        return RMX_OK;
    }
    return fail(c, RMX_E_INVAL, "unknown option '%s'", key);
}

// spectrum scratch of at least `windows` window slots (B * 64 KiB each)
static_assert(host::kSpecBytes4096 == 8 * kThreads * sizeof(float4), "host::plan_caf counts a stored N = 4096 spectrum as 64 KiB");
static int ensure_spec(rmx_ctx* c, long windows) {
    RMX_MEM(c->d_spec.reserve((size_t)windows * c->n_buoys * (8 * kThreads)));
    return RMX_OK;
}

// The call's windows on the device: a device pointer as it is; host windows in the ctx's d_in, with (copy_now) one copy
// up front on the ctx stream
static int host_input(rmx_ctx* c, const void* iq, size_t bytes, bool in_dev, bool copy_now, const void** d_iq) {
    *d_iq = iq;
    if (in_dev) return RMX_OK;
    RMX_MEM(c->d_in.reserve(bytes));
    if (copy_now) RMX_HIP(c, hipMemcpyAsync(c->d_in, iq, bytes, hipMemcpyHostToDevice, c->stream));
    *d_iq = c->d_in;
    return RMX_OK;
}

// host-pointer results: the three arrays live in ONE device block.  Small batches (the seam's one frequency group per
// call) come back as ONE copy into pinned memory + three memcpys instead of three pageable copies (each of which the
// runtime stages and synchronises on its own); large ones keep the three direct copies.
static constexpr size_t kPackedOutMax = 256 * 1024;   // bytes of all three arrays
struct OutBlock {   // views into d_out: four sub-arrays a quarter of its capacity apart
    int* lag;  float* frac;  float* peak;  int* dop;   // (dop: rmx_caf_batch's fourth array)
};
static OutBlock out_block(const rmx_ctx* c) {
    float* base = c->d_out;
    const size_t stride = c->d_out.capacity() / 4;
    return {reinterpret_cast<int*>(base), base + stride, base + 2 * stride, reinterpret_cast<int*>(base + 3 * stride)};
}
static int ensure_out(rmx_ctx* c, size_t out_elems) {
    const size_t stride = (out_elems + 63) & ~(size_t)63;           // 256-byte aligned sub-arrays
    RMX_MEM(c->d_out.reserve(4 * stride));
    return RMX_OK;
}
static int fetch_out(rmx_ctx* c, size_t out_elems, int32_t* lag_int, float* lag_frac, float* peak, int32_t* dop = nullptr) {
    const size_t nb = out_elems * sizeof(float);
    const OutBlock o = out_block(c);
    const char* first = reinterpret_cast<const char*>(o.lag);
    const char* last = reinterpret_cast<const char*>(dop ? (void*)o.dop : (void*)o.peak);
    const size_t span = (size_t)(last - first) + nb;
    if (span <= kPackedOutMax) {
        RMX_MEM(c->h_out.reserve(kPackedOutMax));
        RMX_HIP(c, hipMemcpyAsync(c->h_out, o.lag, span, hipMemcpyDeviceToHost, c->stream));
        RMX_HIP(c, hipStreamSynchronize(c->stream));
        const char* h = c->h_out;
        std::memcpy(lag_int, h, nb);
        std::memcpy(lag_frac, h + (reinterpret_cast<const char*>(o.frac) - first), nb);
        std::memcpy(peak, h + (reinterpret_cast<const char*>(o.peak) - first), nb);
        if (dop) std::memcpy(dop, h + (reinterpret_cast<const char*>(o.dop) - first), nb);
        return RMX_OK;
    }
    if (dop) RMX_HIP(c, hipMemcpyAsync(dop, o.dop, nb, hipMemcpyDeviceToHost, c->stream));
    RMX_HIP(c, hipMemcpyAsync(lag_int, o.lag, nb, hipMemcpyDeviceToHost, c->stream));
    RMX_HIP(c, hipMemcpyAsync(lag_frac, o.frac, nb, hipMemcpyDeviceToHost, c->stream));
    RMX_HIP(c, hipMemcpyAsync(peak, o.peak, nb, hipMemcpyDeviceToHost, c->stream));
    RMX_HIP(c, hipStreamSynchronize(c->stream));
    return RMX_OK;
}

// `elems` int32 of src into s->d through the pinned s->h: the caller may reuse src as soon as the call returns (with
// RMX_OUT_DEVICE too), and the copy runs on the ctx stream -- behind every earlier kernel that reads s->d, in front of
// this call's kernels
static int stage_to_device(rmx_ctx* c, DevStage* s, const int32_t* src, size_t elems) {
    if (!s->ev) RMX_HIP(c, hipEventCreateWithFlags(&s->ev, hipEventDisableTiming));
    RMX_HIP(c, hipEventSynchronize(s->ev));   // the previous call's copy out of the pinned buffer has finished
    RMX_MEM(s->h.reserve(elems));
    RMX_MEM(s->d.reserve(elems));
    std::memcpy(s->h, src, elems * sizeof(int32_t));
    RMX_HIP(c, hipMemcpyAsync(s->d, s->h, elems * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    RMX_HIP(c, hipEventRecord(s->ev, c->stream));
    return RMX_OK;
}

// The second pass of a quality call that asks for nothing else that needs the spectra in HBM (no band, no weighting, no
// integration, no refinement).  Its three lag outputs have just been written by the routes of the SAME call without
// quality -- the whole-window kernels included, which keep their spectra to themselves --, so they are that call's
// outputs bit for bit; here the per-transform forward kernels store the spectra chunk by chunk and k_quality reads them
// and the peaks.  The input is on the device (the caller's, or the ctx's copy the first pass made).
static int quality_pass(rmx_ctx* c, const XcorrCall& req, const void* iq, int n_windows, int n_pairs, float* peak, unsigned flags) {
    const bool in_dev = flags & RMX_IN_DEVICE, out_dev = flags & RMX_OUT_DEVICE, u8 = flags & RMX_IN_U8;
    const void* d_iq = in_dev ? iq : c->d_in.get();
    float* d_peak = out_dev ? peak : out_block(c).peak;
    const size_t out_elems = (size_t)n_windows * n_pairs;
    XcorrCall call = req;
    if (!out_dev) {
        RMX_MEM(c->d_quality.reserve(4 * out_elems));
        call.quality = c->d_quality;
    }
    int rc = c->generic ? rmx::generic_ensure(c, n_pairs, true, true)
                        : ensure_spec(c, n_windows < c->chunk_windows ? n_windows : c->chunk_windows);
    if (rc == RMX_OK)
        rc = run_chunks(c, call, route_caps(c), d_iq, 0, n_windows, c->generic ? c->g_chunk : c->chunk_windows, n_pairs, nullptr, nullptr,
                        d_peak, u8, false);
    if (rc != RMX_OK) return rc;
    if (!out_dev) {
        RMX_HIP(c, hipMemcpyAsync(req.quality, c->d_quality, 4 * out_elems * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        RMX_HIP(c, hipStreamSynchronize(c->stream));
    }
    return RMX_OK;
}

// One correlation call as `call` describes it -- plain, bounded, weighted, integrated or any mix: every route launches the
// instantiations the request names (the bounded one of its peak-searching kernel, lag_bounds.hpp; the weighted one of its
// per-transform forward kernel, xspec_weight.hpp; the integrating one of its pair kernel, integrate.hpp) or, where a
// route has none, is steered to the per-transform kernels.  The arguments have been checked (xcorr_request).
static int xcorr_dispatch(rmx_ctx* c, const XcorrCall& req, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                          int32_t* lag_int, float* lag_frac, float* peak, unsigned flags) {
    // Quality and nothing else that needs the spectra in HBM: the three lag outputs come from the routes of the same call
    // without quality, so they are that call's bit for bit whatever kernel it takes; the figures follow in a second pass.
    // (A banded call runs the per-transform kernels with or without quality: one pass, k_quality behind its pair kernels.)
    if (req.qualified() && !req.wt.band && !req.banded() && !req.integrated() && !req.refined()) {
        XcorrCall lags = req;
        lags.quality = nullptr;
        const int rc_l = xcorr_dispatch(c, lags, iq, n_windows, pairs, n_pairs, lag_int, lag_frac, peak, flags);
        if (rc_l != RMX_OK) return rc_l;
        return quality_pass(c, req, iq, n_windows, n_pairs, peak, flags);
    }
    XcorrCall call = req;   // (req.quality is the caller's pointer; a host-pointer call gets the ctx's device block below)
    tm_reset(c);
    const bool in_dev = flags & RMX_IN_DEVICE, out_dev = flags & RMX_OUT_DEVICE, u8 = flags & RMX_IN_U8;
    // the route (host_plan.hpp: plan_route), and the pair plan with the pairs per workgroup it chose
    const host::RouteCall rq{n_windows, n_pairs, host::is_default_list(c->n_buoys, pairs, n_pairs), pairs != nullptr, call.bounded(),
                             call.weighted(), call.integ, in_dev, call.banded() ? call.bs.n_bands : 1};
    const host::RouteCaps caps = route_caps(c);
    const host::RoutePlan plan = host::plan_route(caps, rq);
    if (!c->generic) c->pairs_per_block = plan.ppb;
    int rc = build_plan(c, pairs, n_pairs);
    if (rc == RMX_OK && !c->generic) rc = route_refusal(c, plan.refused, plan.bands_chunk, caps, call.integ, rq.n_bands);
    if (rc != RMX_OK) return rc;

    const size_t samp_bytes = u8 ? 2 : 8;
    const size_t in_bytes = (size_t)n_windows * c->n_buoys * c->n_samples * samp_bytes;
    // k_win: the copy is cut into sub-chunks issued on a second stream, each followed by its
    // kernel launch, so that copy k+1 travels while kernel k runs (below); otherwise one copy up front
    const void* d_iq = nullptr;
    rc = host_input(c, iq, in_bytes, in_dev, !plan.pipelined, &d_iq);
    if (rc != RMX_OK) return rc;
    if (!in_dev && plan.pipelined) {
        if (!c->copy_stream) RMX_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        for (hipEvent_t& e : c->copy_ev)
            if (!e) RMX_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        // earlier work of this ctx may still read the staging buffer
        RMX_HIP(c, hipEventRecord(c->copy_ev[3], c->stream));
        RMX_HIP(c, hipStreamWaitEvent(c->copy_stream, c->copy_ev[3], 0));
    }
    int* d_lag = lag_int;
    float *d_frac = lag_frac, *d_peak = peak;
    // (integrated call: one row per group; banded call: one row per virtual window, host::plan_bands' out_elems)
    const size_t out_elems = (size_t)(n_windows / call.integ) * n_pairs * (size_t)rq.n_bands;
    if (!out_dev) {
        rc = ensure_out(c, out_elems);
        if (rc != RMX_OK) return rc;
        if (call.qualified()) RMX_MEM(c->d_quality.reserve(4 * out_elems));
        const OutBlock o = out_block(c);
        d_lag = o.lag; d_frac = o.frac; d_peak = o.peak;
        if (call.qualified()) call.quality = c->d_quality;
    }
    // host-pointer results: the fourth array is queued in front of fetch_out, which waits for the stream
    auto done = [&](int rc_k) -> int {
        if (rc_k != RMX_OK || out_dev) return rc_k;
        if (call.qualified())
            RMX_HIP(c, hipMemcpyAsync(req.quality, c->d_quality, 4 * out_elems * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        return fetch_out(c, out_elems, lag_int, lag_frac, peak);
    };
    if (c->generic) return done(rmx::generic_batch(c, call, caps, rq, plan, d_iq, d_lag, d_frac, d_peak, u8));
    const bool k_win_route = plan.route == host::kRouteKWin;
    const long chunk_w = n_windows < c->chunk_windows ? n_windows : c->chunk_windows;
    rc = ensure_spec(c, k_win_route ? (chunk_w < c->n_cus ? chunk_w : c->n_cus) : chunk_w);   // per workgroup for k_win, per window of a chunk otherwise
    if (rc != RMX_OK) return rc;
    if (!k_win_route) return done(run_chunks(c, call, caps, d_iq, 0, n_windows, plan.chunk, n_pairs, d_lag, d_frac, d_peak, u8));
    const float out_scale = out_scale4096();   // (the forward scale 2^-6 rides on the TW1 table)
    int n_sub = 0;
    for (int w0 = 0; w0 < n_windows; w0 += plan.chunk) {
        const int wc = (n_windows - w0 < plan.chunk) ? n_windows - w0 : plan.chunk;
        const int wtail = host::route_wtail4096(caps, plan, n_pairs, w0, wc);   // this chunk's partial round
        const int wf = wc - wtail;
        const int sub = plan.pipelined ? kHostSubChunk : (wf > 0 ? wf : 1);
        for (int s0 = 0; s0 < wf; s0 += sub) {
            const int sc = wf - s0 < sub ? wf - s0 : sub;
            const long wfirst = (long)w0 + s0;
            if (plan.pipelined) {
                const size_t off = (size_t)wfirst * c->n_buoys * c->n_samples * samp_bytes;
                const size_t nb = (size_t)sc * c->n_buoys * c->n_samples * samp_bytes;
                hipEvent_t ev = c->copy_ev[n_sub % 3];
                ++n_sub;
                RMX_HIP(c, hipMemcpyAsync((char*)c->d_in + off, (const char*)iq + off, nb, hipMemcpyHostToDevice,
                                          c->copy_stream));
                RMX_HIP(c, hipEventRecord(ev, c->copy_stream));
                RMX_HIP(c, hipStreamWaitEvent(c->stream, ev, 0));
            }
            // one persistent workgroup per CU (the kernel's LDS footprint allows exactly one)
            const int wgrid = sc < c->n_cus ? sc : c->n_cus;
            rc = with_u8(u8, [&](auto U) {
                constexpr bool U8 = decltype(U)::value;
                auto go = [&](auto kern, auto... lb) {
                    return launch(c, kTkPair4096, kern, dim3(wgrid), dim3(kThreads), kLdsWinBytes, d_iq, c->d_spec, c->d_tw1, c->d_tw2,
                                  c->n_buoys, wfirst, out_scale, d_lag, d_frac, d_peak, sc, reinterpret_cast<const int4*>(c->d_trail.get()), c->stag_kwin, lb...);
                };
#ifdef RMX_EXPERIMENTS
                if (c->win8)
                    return launch(c, kTkPair4096, w8::k_win8<U8>, dim3(wgrid), dim3(w8::kT8), w8::kLdsWin8Bytes, d_iq, c->d_spec, c->d_tw1_8,
                                  c->d_tb8, c->d_tc8, c->n_buoys, wfirst, out_scale, d_lag, d_frac, d_peak, sc, c->stag);
                if (c->pk)
                    return launch(c, kTkPair4096, k_winp<U8>, dim3(wgrid), dim3(kThreads), pk::kLdsWinpBytes, d_iq, c->d_spec, c->d_tw1,
                                  c->d_tw2, c->n_buoys, wfirst, out_scale, d_lag, d_frac, d_peak, sc);
#endif
                return call.bounded() ? go(k_win_lb<U8>, call.lb) : go(k_win<U8>);   // (k_win_lb: k_win's bounded instantiation)
            });
            if (rc != RMX_OK) return rc;
        }
        if (wtail) {
            rc = run_chunks(c, call, caps, d_iq, w0 + wf, wtail, wtail, n_pairs, d_lag, d_frac, d_peak, u8);
            if (rc != RMX_OK) return rc;
        }
    }
    return done(RMX_OK);
}

// ---- the request of one call (host_request.hpp) and its way to the device ------------------------------------------
// The checked request's small host arrays onto the device, through the ctx's own staging (the caller may reuse its arrays
// on return), and into `call`: the bands as signed bins where the call is weighted, the lag intervals where it is
// bounded.  Both the correlation entries (xcorr_request) and the Doppler search (rmx_caf_batch_request) describe their
// call so.
static int describe_call(rmx_ctx* c, const host::Request& rq, XcorrCall* call) {
    if (rq.weighted) {
        const int rc = stage_to_device(c, &c->band_stage, rq.bins.data(), rq.bins.size());
        if (rc != RMX_OK) return rc;
        // band_stage of a banded call: [full band | band set].  PHAT keeps call->wt on the full band (every bin whitened,
        // none dropped); without it the forward kernels are the plain ones
        if (rq.n_bands > 1) call->bs = BandSet{c->band_stage.d + 2, rq.band_per_window ? 2L * rq.n_bands : 0L, 0L, rq.n_bands};
        if (rq.n_bands == 1 || rq.phat)
            call->wt = XWeight{c->band_stage.d, rq.n_bands == 1 && rq.band_per_window ? 2L : 0L, 0L, c->n_buoys, rq.phat ? 1 : 0, 1.0f};
    }
    if (rq.bounded) {
        const int rc = stage_to_device(c, &c->lb_stage, rq.bounds, (size_t)(2 * rq.bound_rows));
        if (rc != RMX_OK) return rc;
        call->lb = LagBounds{c->lb_stage.d, rq.bounds_per_window ? 2L * rq.n_pairs : 0L, 0L, rq.n_pairs};
    }
    return RMX_OK;
}

// What all nine correlation entries do, and none of them through another: hand their arguments to host::check_request
// -- every refusal, in one order whichever entry the call came through --, copy the bands (as signed bins) and the lag
// intervals into ctx-owned device buffers, describe the call in an XcorrCall and dispatch it.  The plain call is
// integrate = 1, no band, no weighting, no bounds.
static int xcorr_request(rmx_ctx* c, host::RequestArgs a, unsigned flags) {
    if (!c) return RMX_E_INVAL;
    a.n_buoys = c->n_buoys;
    a.n_samples = c->n_samples;
    a.max_windows = c->max_windows;
    a.flags = flags;
    host::Request rq;
    std::string why;
    int rc = host::check_request(a, &rq, &why);
    if (rc != RMX_OK) return fail(c, rc, "%s", why.c_str());
    if (rq.empty) return RMX_OK;
    RMX_HIP(c, hipSetDevice(c->device));
    XcorrCall call;
    call.integ = rq.integ;
    call.refine = rq.refine;
    call.quality = a.quality;
    rc = describe_call(c, rq, &call);
    if (rc != RMX_OK) return rc;
    return xcorr_dispatch(c, call, a.iq, a.n_windows, a.pairs, rq.n_pairs, a.lag_int, a.lag_frac, a.peak, flags);
}

// the arguments every correlation entry takes
static host::RequestArgs batch_args(const void* iq, int n_windows, const int32_t* pairs, int n_pairs, int32_t* lag_int, float* lag_frac,
                                    float* peak) {
    host::RequestArgs a;
    a.iq = iq;
    a.n_windows = n_windows;
    a.pairs = pairs;
    a.n_pairs = n_pairs;
    a.lag_int = lag_int;
    a.lag_frac = lag_frac;
    a.peak = peak;
    return a;
}
// ... and what the weighted entry adds, which every entry behind it takes too
static host::RequestArgs weighted_args(host::RequestArgs a, const double* band_cps, int band_per_window, unsigned weighting,
                                       const int32_t* lag_bounds, int bounds_per_window) {
    a.band_cps = band_cps;
    a.band_per_window = band_per_window;
    a.weighting = weighting;
    a.lag_bounds = lag_bounds;
    a.bounds_per_window = bounds_per_window;
    return a;
}

int rmx_xcorr_batch(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                    int32_t* lag_int, float* lag_frac, float* peak, unsigned flags) {
    return xcorr_request(c, batch_args(iq, n_windows, pairs, n_pairs, lag_int, lag_frac, peak), flags);
}

// rmx_xcorr_batch with a lag interval per (window, pair).  Every interval the full one IS the plain call.
int rmx_xcorr_batch_bounded(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                            const int32_t* lag_bounds, int bounds_per_window, int32_t* lag_int, float* lag_frac, float* peak,
                            unsigned flags) {
    host::RequestArgs a = batch_args(iq, n_windows, pairs, n_pairs, lag_int, lag_frac, peak);
    a.bounds_required = true;
    a.lag_bounds = lag_bounds;
    a.bounds_per_window = bounds_per_window;
    return xcorr_request(c, a, flags);
}

// rmx_xcorr_batch(_bounded) on band-masked and / or PHAT-whitened spectra.  No band (or the full one) and no weighting IS
// the bounded or the plain call.
int rmx_xcorr_batch_weighted(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                             const double* band_cps, int band_per_window, unsigned weighting,
                             const int32_t* lag_bounds, int bounds_per_window,
                             int32_t* lag_int, float* lag_frac, float* peak, unsigned flags) {
    return xcorr_request(c, weighted_args(batch_args(iq, n_windows, pairs, n_pairs, lag_int, lag_frac, peak), band_cps, band_per_window,
                                          weighting, lag_bounds, bounds_per_window), flags);
}

// rmx_xcorr_batch_weighted under n_bands bands per window over ONE set of forward spectra (xspec_bands.hpp): the forward
// kernels run unmasked -- plain, or under PHAT weighted with the full band --, the kernels that form the product mask it,
// and the pair kernels see n_windows * n_bands virtual windows.  n_bands = 1 IS the weighted call.
int rmx_xcorr_batch_bands(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                          const double* band_cps, int n_bands, int bands_per_window, unsigned weighting,
                          const int32_t* lag_bounds, int bounds_per_window,
                          int32_t* lag_int, float* lag_frac, float* peak, unsigned flags) {
    host::RequestArgs a = weighted_args(batch_args(iq, n_windows, pairs, n_pairs, lag_int, lag_frac, peak), band_cps, bands_per_window,
                                        weighting, lag_bounds, bounds_per_window);
    a.banded = true;
    a.n_bands = n_bands;
    return xcorr_request(c, a, flags);
}

// rmx_xcorr_batch_weighted with one peak search per group of `integrate` consecutive windows, on the lag-by-lag sum of the
// windows' |c|^2 (integrate.hpp): the bands stay per window, the bounds and the outputs are per group.  integrate = 1 IS
// the weighted call.
int rmx_xcorr_batch_integrated(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs, int integrate,
                               const double* band_cps, int band_per_window, unsigned weighting,
                               const int32_t* lag_bounds, int bounds_per_group,
                               int32_t* lag_int, float* lag_frac, float* peak, unsigned flags) {
    host::RequestArgs a = weighted_args(batch_args(iq, n_windows, pairs, n_pairs, lag_int, lag_frac, peak), band_cps, band_per_window,
                                        weighting, lag_bounds, bounds_per_group);
    a.grouped = true;
    a.integrate = integrate;
    return xcorr_request(c, a, flags);
}

// rmx_xcorr_batch_integrated with the fine lag search of refine.hpp behind the coarse one: refine = U in {2, 4, 8, 16}
// relocates each estimate within +-1 sample of the integer peak the coarse rule chose.  refine = 0 IS the integrated call.
int rmx_xcorr_batch_refined(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs, int integrate,
                            const double* band_cps, int band_per_window, unsigned weighting,
                            const int32_t* lag_bounds, int bounds_per_group, int refine,
                            int32_t* lag_int, float* lag_frac, float* peak, unsigned flags) {
    host::RequestArgs a = weighted_args(batch_args(iq, n_windows, pairs, n_pairs, lag_int, lag_frac, peak), band_cps, band_per_window,
                                        weighting, lag_bounds, bounds_per_group);
    a.grouped = true;
    a.integrate = integrate;
    a.refine = refine;
    return xcorr_request(c, a, flags);
}

// rmx_xcorr_batch_refined with four quality figures per output slot (quality.hpp) as a fourth output, computed from the
// pair's two stored spectra and the coarse peak.  quality == NULL IS the refined call.
int rmx_xcorr_batch_quality(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs, int integrate,
                            const double* band_cps, int band_per_window, unsigned weighting,
                            const int32_t* lag_bounds, int bounds_per_group, int refine,
                            int32_t* lag_int, float* lag_frac, float* peak, float* quality, unsigned flags) {
    host::RequestArgs a = weighted_args(batch_args(iq, n_windows, pairs, n_pairs, lag_int, lag_frac, peak), band_cps, band_per_window,
                                        weighting, lag_bounds, bounds_per_group);
    a.grouped = true;
    a.integrate = integrate;
    a.refine = refine;
    a.quality = quality;
    return xcorr_request(c, a, flags);
}

// rmx_xcorr_batch_bands with the fine lag search and the quality figures of rmx_xcorr_batch_quality per (window, band,
// pair): k_quality, then k_refine, behind every chunk's pair kernels in their banded instantiations (refine.hpp,
// quality.hpp), which read the chunk's unmasked spectra under the slot's band.  No forward pass is added.  refine == 0 and
// quality == NULL IS rmx_xcorr_batch_bands; n_bands == 1 IS rmx_xcorr_batch_quality with integrate = 1.
int rmx_xcorr_batch_bands_quality(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                                  const double* band_cps, int n_bands, int bands_per_window, unsigned weighting,
                                  const int32_t* lag_bounds, int bounds_per_window, int refine,
                                  int32_t* lag_int, float* lag_frac, float* peak, float* quality, unsigned flags) {
    host::RequestArgs a = weighted_args(batch_args(iq, n_windows, pairs, n_pairs, lag_int, lag_frac, peak), band_cps, bands_per_window,
                                        weighting, lag_bounds, bounds_per_window);
    a.banded = true;
    a.n_bands = n_bands;
    a.refine = refine;
    a.quality = quality;
    return xcorr_request(c, a, flags);
}

// rmx_xcorr_batch_bands_quality with one peak search per (group of `integrate` consecutive windows, band): the banded
// integrating instantiations of the pair kernels, of k_quality and of k_refine (xspec_bands.hpp) walk each group's real
// windows under the band of each window.  integrate == 1 IS rmx_xcorr_batch_bands_quality; n_bands == 1 IS
// rmx_xcorr_batch_quality.
int rmx_xcorr_batch_bands_integrated(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs, int integrate,
                                     const double* band_cps, int n_bands, int bands_per_window, unsigned weighting,
                                     const int32_t* lag_bounds, int bounds_per_group, int refine,
                                     int32_t* lag_int, float* lag_frac, float* peak, float* quality, unsigned flags) {
    host::RequestArgs a = weighted_args(batch_args(iq, n_windows, pairs, n_pairs, lag_int, lag_frac, peak), band_cps, bands_per_window,
                                        weighting, lag_bounds, bounds_per_group);
    a.grouped = true;
    a.integrate = integrate;
    a.banded = true;
    a.n_bands = n_bands;
    a.refine = refine;
    a.quality = quality;
    return xcorr_request(c, a, flags);
}

// ---- the Doppler search (host_plan.hpp: plan_caf decides its shape; this executes it) -----------------------------------------
// One search on its way to the device.  `call` describes the search's own forward and pair kernels and is never refined
// or qualified: they are those of rmx_caf_batch_request whatever else is asked.  `tail` is what follows the selection:
// call + refine + quality, the quality pointer the ctx's block for a host-pointer call.  The five outputs as the kernels
// write them: the caller's device arrays, or the ctx's blocks.
struct CafRun {
    XcorrCall call, tail;
    const void* d_iq = nullptr;
    int n_windows = 0, n_pairs = 0, n_dopplers = 0;
    bool u8 = false;
    int *dop = nullptr, *lag = nullptr;
    float *frac = nullptr, *peak = nullptr, *dfrac = nullptr;   // (dfrac: NULL unless dop_frac is asked for)
};

// phasor table [D][N] under the grid: exp(-2 pi i nu n) in double, rounded once to float
static int caf_phasors(rmx_ctx* c, const double* doppler_cps, int n_dopplers) {
    const int N = c->n_samples;
    std::vector<double> grid(doppler_cps, doppler_cps + n_dopplers);
    if (c->caf_rot.holds(grid)) return RMX_OK;
    std::vector<float2> rot((size_t)n_dopplers * N);
    for (int d = 0; d < n_dopplers; ++d)
        for (int n = 0; n < N; ++n) {
            const double a = -6.283185307179586476925286766559 * grid[d] * (double)n;
            rot[(size_t)d * N + n] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
    RMX_MEM(c->caf_rot.refill(grid, rot));
    return RMX_OK;
}

// The buffers the plan sizes -- the per-hypothesis results, the outputs of a host-pointer call, k_caf_select_fd's
// neighbour rows with the staged dop_frac behind them, the staged quality -- and where `r` writes its outputs
static int caf_buffers(rmx_ctx* c, const host::RequestArgs& a, const host::CafPlan& plan, bool out_dev, CafRun* r) {
    RMX_MEM(c->caf_lag.reserve(plan.hyp_elems));
    RMX_MEM(c->caf_frac.reserve(plan.hyp_elems));
    RMX_MEM(c->caf_peak.reserve(plan.hyp_elems));
    r->dop = a.dop_idx; r->lag = a.lag_int; r->frac = a.lag_frac; r->peak = a.peak; r->dfrac = a.dop_frac;
    if (!out_dev) {
        const int rc = ensure_out(c, plan.out_elems);
        if (rc != RMX_OK) return rc;
        const OutBlock o = out_block(c);
        r->dop = o.dop; r->lag = o.lag; r->frac = o.frac; r->peak = o.peak;
    }
    if (plan.need_nb) RMX_MEM(c->caf_nb.reserve(4 * plan.out_elems));
    if (plan.stage_dfrac) r->dfrac = c->caf_nb + 3 * plan.out_elems;
    if (a.quality && !out_dev) {
        RMX_MEM(c->d_quality.reserve(4 * plan.out_elems));
        r->tail.quality = c->d_quality;
    }
    return RMX_OK;
}

// N = 4096, one chunk: all hypotheses in ONE forward launch and ONE pair launch (virtual window = hypothesis x window)
// instead of three launches per hypothesis, ONE selection over the resident per-hypothesis results, and the tail once
static int caf_one_launch(rmx_ctx* c, const CafRun& r, const host::CafPlan& plan) {
    const int W = r.n_windows, D = r.n_dopplers;
    const SpecView sv = spec_view(c);
    int rc = fwd4096(c, r.call, r.d_iq, 0, W, r.u8, nullptr);
    if (rc == RMX_OK) rc = fwd4096(c, r.call, r.d_iq, 0, W, r.u8, c->caf_rot, D);
    if (rc == RMX_OK) rc = pairs4096(c, r.call, 0, W, r.n_pairs, c->caf_lag, c->caf_frac, c->caf_peak, out_scale4096(), true, D);
    const dim3 sgrid((unsigned)((plan.out_elems + 255) / 256));
    if (rc == RMX_OK && !r.dfrac)
        rc = launch(c, kTkCafSelect, k_caf_select_all, sgrid, dim3(256), 0, D, (long)plan.out_elems, c->caf_lag, c->caf_frac, c->caf_peak,
                    r.dop, r.lag, r.frac, r.peak);
    if (rc == RMX_OK && r.dfrac)
        rc = launch(c, kTkCafSelect, k_caf_select_all_fd, sgrid, dim3(256), 0, D, (long)plan.out_elems, c->caf_lag, c->caf_frac, c->caf_peak,
                    r.dop, r.lag, r.frac, r.peak, r.dfrac);
    // every de-rotated set is resident: slot (w, q) reads operand j at virtual window dop_idx * W + w (a group's slot
    // (g, q): at dop_idx * W + g K + kw, its K windows in order)
    const CafWinner cw{r.dop, reinterpret_cast<const float2*>(c->d_spec_r.get()), (long)W * c->n_buoys, -1};
    if (rc == RMX_OK && r.tail.qualified()) rc = quality_chunk(c, r.tail, sv, 0, W, r.n_pairs, r.peak, &cw);
    if (rc == RMX_OK && r.tail.refined()) rc = refine_chunk(c, r.tail, sv, 0, W, r.n_pairs, r.lag, r.frac, r.peak, &cw);
    return rc;
}

// Per chunk of windows: the un-rotated spectra once, then per hypothesis the de-rotated spectra (the rotation is applied
// as the window is loaded), the pair kernels with X_i un-rotated and X_j de-rotated, and the running d-major first
// maximum.  No augmented copy of the windows, no second engine.
static int caf_sweep(rmx_ctx* c, const CafRun& r, const host::CafPlan& plan) {
    const int K = r.call.integ, N = c->n_samples, D = r.n_dopplers;
    const SpecView sv = spec_view(c);
    int rc = RMX_OK;
    for (int w0 = 0; w0 < r.n_windows && rc == RMX_OK; w0 += plan.chunk) {
        const int wc = r.n_windows - w0 < plan.chunk ? r.n_windows - w0 : plan.chunk;
        rc = sv.forward(c, r.call, r.d_iq, w0, wc, r.u8, nullptr, false);
        for (int d = 0; d < D && rc == RMX_OK; ++d) {
            rc = sv.forward(c, r.call, r.d_iq, w0, wc, r.u8, c->caf_rot + (size_t)d * N, false);
            if (rc != RMX_OK) break;
            rc = sv.pairs(c, r.call, w0, wc, r.n_pairs, c->caf_lag, c->caf_frac, c->caf_peak, true, false);
            if (rc != RMX_OK) break;
            // the chunk's output rows (banded: n_bands virtual windows per window, never integrated)
            const long nb = r.call.banded() ? r.call.bs.n_bands : 1;
            const long first = (long)(w0 / K) * nb * r.n_pairs, cnt = (long)(wc / K) * nb * r.n_pairs;
            const dim3 sgrid((unsigned)((cnt + 255) / 256));
            if (r.dfrac)
                rc = launch(c, kTkCafSelect, k_caf_select_fd, sgrid, dim3(256), 0, d, D, first, cnt, (long)plan.out_elems, c->caf_lag,
                            c->caf_frac, c->caf_peak, r.dop, r.lag, r.frac, r.peak, c->caf_nb, r.dfrac);
            else
                rc = launch(c, kTkCafSelect, k_caf_select, sgrid, dim3(256), 0, d, first, cnt, c->caf_lag, c->caf_frac, c->caf_peak, r.dop,
                            r.lag, r.frac, r.peak);
        }
        // The chunk's winners are known now and only the last hypothesis' de-rotated set is left: the hypotheses once
        // more, each followed by k_quality and k_refine on the slots it won (k_quality in front: k_refine overwrites peak)
        for (int d = 0; plan.second_sweep && d < D && rc == RMX_OK; ++d) {
            rc = sv.forward(c, r.call, r.d_iq, w0, wc, r.u8, c->caf_rot + (size_t)d * N, false);
            const CafWinner cw{r.dop, c->generic ? c->g_spec_r.get() : reinterpret_cast<const float2*>(c->d_spec_r.get()), 0L, d};
            if (rc == RMX_OK && r.tail.qualified()) rc = quality_chunk(c, r.tail, sv, w0, wc, r.n_pairs, r.peak, &cw);
            if (rc == RMX_OK && r.tail.refined()) rc = refine_chunk(c, r.tail, sv, w0, wc, r.n_pairs, r.lag, r.frac, r.peak, &cw);
        }
    }
    return rc;
}

// What all five Doppler entries do, and none of them through another: hand their arguments to host::check_caf_request --
// every refusal, in one order whichever entry the call came through --, describe the search in an XcorrCall (the staged
// bands and lag intervals), let host::plan_caf decide its shape and run that.  The plain search is one window per group,
// no band, no weighting, no bounds, dop_frac == NULL, nothing refined or qualified.
static int caf_request(rmx_ctx* c, host::RequestArgs a, unsigned flags) {
    if (!c) return RMX_E_INVAL;
    a.n_buoys = c->n_buoys;
    a.n_samples = c->n_samples;
    a.max_windows = c->max_windows;
    a.flags = flags;
    a.grouped = true;
    host::Request rq;
    std::string why;
    int rc = host::check_caf_request(a, &rq, &why);
    if (rc != RMX_OK) return fail(c, rc, "%s", why.c_str());
    if (rq.empty) return RMX_OK;
    RMX_HIP(c, hipSetDevice(c->device));
    const bool in_dev = flags & RMX_IN_DEVICE, out_dev = flags & RMX_OUT_DEVICE;
    CafRun r;
    r.n_windows = a.n_windows;  r.n_pairs = rq.n_pairs;  r.n_dopplers = a.n_dopplers;  r.u8 = flags & RMX_IN_U8;
    r.call.integ = rq.integ;
    rc = describe_call(c, rq, &r.call);
    if (rc != RMX_OK) return rc;
    r.tail = r.call;
    r.tail.refine = rq.refine;
    r.tail.quality = a.quality;
    const host::CafCall cq{a.n_windows, rq.n_pairs, a.n_dopplers, rq.integ, a.dop_frac != nullptr, r.tail.refined(), r.tail.qualified(),
                           out_dev, rq.n_bands};
    host::RouteCaps caps = route_caps(c);
    host::CafPlan plan = host::plan_caf(caps, cq);
    if (!c->generic) c->pairs_per_block = plan.ppb;   // (N = 4096: blocks sized to this batch, not to the previous call's)
    rc = build_plan(c, a.pairs, rq.n_pairs);
    if (rc == RMX_OK) rc = route_refusal(c, plan.refused, 0, caps, rq.integ, rq.n_bands, rq.n_pairs);
    if (rc == RMX_OK) rc = host_input(c, a.iq, (size_t)a.n_windows * c->n_buoys * c->n_samples * (r.u8 ? 2 : 8), in_dev, true, &r.d_iq);
    if (rc == RMX_OK) rc = caf_phasors(c, a.doppler_cps, a.n_dopplers);
    if (rc == RMX_OK) rc = caf_buffers(c, a, plan, out_dev, &r);
    if (rc != RMX_OK) return rc;
    tm_reset(c);
    if (c->generic) {   // a failed allocation halves g_chunk, and the plan follows: whole groups per chunk, or the refusal
        rc = rmx::generic_ensure(c, rq.n_pairs, true, true, rq.n_bands);
        if (rc == RMX_OK && c->g_chunk != caps.g_chunk) {
            caps.g_chunk = c->g_chunk;
            plan = host::plan_caf(caps, cq);
            rc = route_refusal(c, plan.refused, 0, caps, rq.integ, rq.n_bands, rq.n_pairs);
        }
    } else {
        rc = ensure_spec(c, a.n_windows < c->chunk_windows ? a.n_windows : c->chunk_windows);
    }
    if (rc == RMX_OK) rc = plan.one_launch ? caf_one_launch(c, r, plan) : caf_sweep(c, r, plan);
    if (rc != RMX_OK || out_dev) return rc;
    // host-pointer results: dop_frac and quality are queued in front of fetch_out, which waits for the stream
    if (a.dop_frac) RMX_HIP(c, hipMemcpyAsync(a.dop_frac, r.dfrac, plan.out_elems * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (a.quality) RMX_HIP(c, hipMemcpyAsync(a.quality, r.tail.quality, 4 * plan.out_elems * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return fetch_out(c, plan.out_elems, a.lag_int, a.lag_frac, a.peak, a.dop_idx);
}

// the arguments every Doppler entry takes: batch_args, the grid and the search's own two outputs
static host::RequestArgs caf_args(const void* iq, int n_windows, const int32_t* pairs, int n_pairs, const double* doppler_cps, int n_dopplers,
                                  int32_t* dop_idx, float* dop_frac, int32_t* lag_int, float* lag_frac, float* peak) {
    host::RequestArgs a = batch_args(iq, n_windows, pairs, n_pairs, lag_int, lag_frac, peak);
    a.doppler_cps = doppler_cps;
    a.n_dopplers = n_dopplers;
    a.dop_idx = dop_idx;
    a.dop_frac = dop_frac;
    return a;
}

int rmx_caf_batch(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                  const double* doppler_cps, int n_dopplers, int32_t* dop_idx, int32_t* lag_int, float* lag_frac,
                  float* peak, unsigned flags) {
    return caf_request(c, caf_args(iq, n_windows, pairs, n_pairs, doppler_cps, n_dopplers, dop_idx, nullptr, lag_int, lag_frac, peak), flags);
}

// The Doppler search under a request: a band and PHAT on every stored spectrum, the rotated ones included, lag intervals
// in every hypothesis' peak search, and (dop_frac) the parabola through the winner's and its two neighbours' peaks.
// Nothing requested IS rmx_caf_batch.
int rmx_caf_batch_request(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                          const double* doppler_cps, int n_dopplers,
                          const double* band_cps, int band_per_window, unsigned weighting,
                          const int32_t* lag_bounds, int bounds_per_window,
                          int32_t* dop_idx, float* dop_frac,
                          int32_t* lag_int, float* lag_frac, float* peak, unsigned flags) {
    return caf_request(c, weighted_args(caf_args(iq, n_windows, pairs, n_pairs, doppler_cps, n_dopplers, dop_idx, dop_frac, lag_int, lag_frac, peak),
                                        band_cps, band_per_window, weighting, lag_bounds, bounds_per_window), flags);
}

// rmx_caf_batch_request with the fine lag search and the quality figures of rmx_xcorr_batch_quality on each slot's WINNING
// hypothesis: behind the selection, k_quality and then k_refine in their <CafWinner> instantiations (caf_select.hpp) read
// operand i from the un-rotated spectra and operand j from the winner's de-rotated ones.  Where every hypothesis' set is
// resident (the one-launch path of N = 4096) that is one launch of each; elsewhere the hypotheses of a chunk are swept a
// second time, each forward pass followed by the two kernels, whose workgroups return unless their slot's winner is resident.
// refine == 0 and quality == NULL IS rmx_caf_batch_request.
int rmx_caf_batch_quality(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                          const double* doppler_cps, int n_dopplers,
                          const double* band_cps, int band_per_window, unsigned weighting,
                          const int32_t* lag_bounds, int bounds_per_window, int refine,
                          int32_t* dop_idx, float* dop_frac,
                          int32_t* lag_int, float* lag_frac, float* peak, float* quality, unsigned flags) {
    host::RequestArgs a = weighted_args(caf_args(iq, n_windows, pairs, n_pairs, doppler_cps, n_dopplers, dop_idx, dop_frac, lag_int, lag_frac, peak),
                                        band_cps, band_per_window, weighting, lag_bounds, bounds_per_window);
    a.refine = refine;
    a.quality = quality;
    return caf_request(c, a, flags);
}

// The Doppler search integrated noncoherently over groups of K = `integrate` consecutive windows: coherent per window
// under each hypothesis, |r|^2 summed over the group's windows, ONE peak search per (group, pair, hypothesis).  The
// forward kernels are the search's; the pair kernels are the integrating instantiations with operand j from the
// de-rotated set (pack <LagBounds, Integrate, CafOperand>, integrate.hpp; the four-step row kernels take spec_j as they
// are and g_cols_inv's integrating instantiation sums their products); the selection runs on G * n_pairs slots; k_quality
// and k_refine <CafWinner> walk the group's windows.  integrate == 1 IS rmx_caf_batch_quality: none of the above is reached.
int rmx_caf_batch_integrated(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                             const double* doppler_cps, int n_dopplers, int integrate,
                             const double* band_cps, int band_per_window, unsigned weighting,
                             const int32_t* lag_bounds, int bounds_per_group, int refine,
                             int32_t* dop_idx, float* dop_frac,
                             int32_t* lag_int, float* lag_frac, float* peak, float* quality, unsigned flags) {
    host::RequestArgs a = weighted_args(caf_args(iq, n_windows, pairs, n_pairs, doppler_cps, n_dopplers, dop_idx, dop_frac, lag_int, lag_frac, peak),
                                        band_cps, band_per_window, weighting, lag_bounds, bounds_per_group);
    a.integrate = integrate;
    a.refine = refine;
    a.quality = quality;
    return caf_request(c, a, flags);
}

// rmx_caf_batch_request under n_bands bands per window over ONE set of forward passes (xspec_bands.hpp): the forward
// kernels run unmasked -- plain, or under PHAT weighted with the full band --, once un-rotated and once per hypothesis
// de-rotated; the banded pair kernels mask the product with operand j from the de-rotated set and see n_bands virtual
// windows per (hypothesis, window); the selection runs over n_windows * n_bands * n_pairs slots.  n_bands == 1 IS
// rmx_caf_batch_request.
int rmx_caf_batch_bands(rmx_ctx* c, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                        const double* doppler_cps, int n_dopplers,
                        const double* band_cps, int n_bands, int bands_per_window, unsigned weighting,
                        const int32_t* lag_bounds, int bounds_per_window,
                        int32_t* dop_idx, float* dop_frac,
                        int32_t* lag_int, float* lag_frac, float* peak, unsigned flags) {
    host::RequestArgs a = weighted_args(caf_args(iq, n_windows, pairs, n_pairs, doppler_cps, n_dopplers, dop_idx, dop_frac, lag_int, lag_frac, peak),
                                        band_cps, bands_per_window, weighting, lag_bounds, bounds_per_window);
    a.banded = true;
    a.n_bands = n_bands;
    return caf_request(c, a, flags);
}

// What rmx_solve_batch_fix asks beyond rmx_solve_batch: the plane (or NULL: three unknowns) and the outputs at the fix.
struct SolveFixArgs {
    const double* plane;
    double *info, *cov, *resid;
};

// The body of both solve entries.  fx == nullptr IS rmx_solve_batch: the same checks, copies and the one k_solve launch.
static int solve_request(rmx_ctx* c, const double* buoy_xyz, int n_buoys, const int32_t* pairs, int n_pairs,
                         const int32_t* lag_int, const float* lag_frac, const float* weight, double sample_rate_hz,
                         int n_windows, int max_iter, double* pos, double* cost, int32_t* iters, unsigned flags,
                         const SolveFixArgs* fx) {
    if (!c) return RMX_E_INVAL;
    if (!buoy_xyz || !lag_int || !lag_frac || !pos || !cost || !iters) return fail(c, RMX_E_INVAL, "NULL buffer");
    if (fx && (!fx->info || !fx->cov)) return fail(c, RMX_E_INVAL, "NULL buffer (info, cov)");
    if (n_buoys < 2 || n_buoys > rmx::kSolveMaxBuoys)
        return fail(c, RMX_E_INVAL, "n_buoys %d not in 2..%d", n_buoys, rmx::kSolveMaxBuoys);
    if (!(sample_rate_hz > 0.0)) return fail(c, RMX_E_INVAL, "sample_rate_hz must be positive");
    if (n_windows < 0 || max_iter < 1) return fail(c, RMX_E_INVAL, "n_windows %d, max_iter %d", n_windows, max_iter);
    const int all_pairs = n_buoys * (n_buoys - 1) / 2;
    std::vector<int32_t> pl;
    if (!pairs) {
        if (n_pairs != 0 && n_pairs != all_pairs)
            return fail(c, RMX_E_INVAL, "pairs == NULL needs n_pairs == 0 or %d, got %d", all_pairs, n_pairs);
        n_pairs = all_pairs;
        for (int i = 0; i < n_buoys; ++i)
            for (int j = i + 1; j < n_buoys; ++j) { pl.push_back(i); pl.push_back(j); }
    } else {
        if (n_pairs < 1 || n_pairs > rmx::kSolveMaxPairs) return fail(c, RMX_E_INVAL, "n_pairs %d out of range", n_pairs);
        for (int q = 0; q < 2 * n_pairs; ++q) {
            if (pairs[q] < 0 || pairs[q] >= n_buoys) return fail(c, RMX_E_INVAL, "pair %d out of range", q / 2);
            pl.push_back(pairs[q]);
        }
    }
    // the new entry's own refusals come behind rmx_solve_batch's, so a call that is wrong in both ways reads the same there
    rmx::SolvePlane spl{};
    if (fx && fx->plane) {
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(fx->plane[k])) return fail(c, RMX_E_INVAL, "plane[%d] is not finite", k);
        const double *e1 = fx->plane + 3, *e2 = fx->plane + 6;
        const double n1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
        const double n2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
        const double dot = e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2];
        if (!(std::fabs(n1 - 1.0) <= 1e-9) || !(std::fabs(n2 - 1.0) <= 1e-9))
            return fail(c, RMX_E_INVAL, "plane: |e1| = %.12g, |e2| = %.12g, both must be 1 to 1e-9", n1, n2);
        if (!(std::fabs(dot) <= 1e-9)) return fail(c, RMX_E_INVAL, "plane: e1 . e2 = %.3g, must be 0 to 1e-9", dot);
        for (int k = 0; k < 3; ++k) { spl.o[k] = fx->plane[k]; spl.e1[k] = e1[k]; spl.e2[k] = e2[k]; }
    }
    if (n_windows == 0) return RMX_OK;
    RMX_HIP(c, hipSetDevice(c->device));
    RMX_MEM(c->sv_buoys.reserve(rmx::kSolveMaxBuoys * 3));
    RMX_MEM(c->sv_pairs.reserve(pl.size()));
    // (pageable host sources: these copies are synchronous with respect to the host buffers)
    RMX_HIP(c, hipMemcpyAsync(c->sv_buoys, buoy_xyz, (size_t)n_buoys * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    RMX_HIP(c, hipMemcpyAsync(c->sv_pairs, pl.data(), pl.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    RMX_HIP(c, hipStreamSynchronize(c->stream));
    const bool in_dev = flags & RMX_IN_DEVICE, out_dev = flags & RMX_OUT_DEVICE;
    const size_t ne = (size_t)n_windows * n_pairs;
    const int* d_li = lag_int;
    const float* d_lf = lag_frac;
    const float* d_wg = weight;
    if (!in_dev) {
        RMX_MEM(c->sv_in.reserve(ne * 4 * 3));
        char* base = c->sv_in;
        RMX_HIP(c, hipMemcpyAsync(base, lag_int, ne * 4, hipMemcpyHostToDevice, c->stream));
        RMX_HIP(c, hipMemcpyAsync(base + ne * 4, lag_frac, ne * 4, hipMemcpyHostToDevice, c->stream));
        if (weight) RMX_HIP(c, hipMemcpyAsync(base + ne * 8, weight, ne * 4, hipMemcpyHostToDevice, c->stream));
        d_li = (const int*)base;
        d_lf = (const float*)(base + ne * 4);
        d_wg = weight ? (const float*)(base + ne * 8) : nullptr;
    }
    double *d_pos = pos, *d_cost = cost;
    int* d_it = iters;
    // the outputs at the fix: n_sym doubles a window for info and for cov, n_pairs for resid where it is asked for
    const bool plane = fx && fx->plane;
    const size_t n_sym = !fx ? 0 : plane ? 3 : 6, n_res = fx && fx->resid ? (size_t)n_pairs : 0;
    double *d_info = fx ? fx->info : nullptr, *d_cov = fx ? fx->cov : nullptr, *d_res = fx ? fx->resid : nullptr;
    if (!out_dev) {
        RMX_MEM(c->sv_out.reserve((size_t)n_windows * ((3 + 1 + 2 * n_sym + n_res) * 8 + 4)));
        d_pos = reinterpret_cast<double*>(c->sv_out.get());
        d_cost = d_pos + (size_t)n_windows * 3;
        double* end = d_cost + n_windows;
        if (fx) {
            d_info = end;
            d_cov = d_info + (size_t)n_windows * n_sym;
            end = d_cov + (size_t)n_windows * n_sym;
            if (n_res) { d_res = end; end += (size_t)n_windows * n_res; }
        }
        d_it = (int*)end;
    }
    const dim3 grid((n_windows + 63) / 64), block(64);
    const double mps = 299792458.0 / sample_rate_hz;
    int rc_k;
    if (plane)
        rc_k = launch(c, kTkNone, k_solve_plane, grid, block, 0, c->sv_buoys, n_buoys, c->sv_pairs, n_pairs, d_li, d_lf, d_wg, mps, spl,
                      n_windows, max_iter, d_pos, d_cost, d_it);
    else
        rc_k = launch(c, kTkNone, k_solve, grid, block, 0, c->sv_buoys, n_buoys, c->sv_pairs, n_pairs, d_li, d_lf,
                      d_wg, mps, n_windows, max_iter, d_pos, d_cost, d_it);
    if (rc_k != RMX_OK) return rc_k;
    if (fx) {
        auto* const k_fix = plane ? &k_solve_fix<true> : &k_solve_fix<false>;
        rc_k = launch(c, kTkNone, k_fix, grid, block, 0, c->sv_buoys, n_buoys, c->sv_pairs, n_pairs, d_li, d_lf, d_wg, mps, spl, n_windows,
                      d_pos, d_info, d_cov, d_res);
        if (rc_k != RMX_OK) return rc_k;
    }
    if (!out_dev) {
        RMX_HIP(c, hipMemcpyAsync(pos, d_pos, (size_t)n_windows * 3 * 8, hipMemcpyDeviceToHost, c->stream));
        RMX_HIP(c, hipMemcpyAsync(cost, d_cost, (size_t)n_windows * 8, hipMemcpyDeviceToHost, c->stream));
        RMX_HIP(c, hipMemcpyAsync(iters, d_it, (size_t)n_windows * 4, hipMemcpyDeviceToHost, c->stream));
        if (fx) {
            RMX_HIP(c, hipMemcpyAsync(fx->info, d_info, (size_t)n_windows * n_sym * 8, hipMemcpyDeviceToHost, c->stream));
            RMX_HIP(c, hipMemcpyAsync(fx->cov, d_cov, (size_t)n_windows * n_sym * 8, hipMemcpyDeviceToHost, c->stream));
            if (n_res) RMX_HIP(c, hipMemcpyAsync(fx->resid, d_res, (size_t)n_windows * n_res * 8, hipMemcpyDeviceToHost, c->stream));
        }
        RMX_HIP(c, hipStreamSynchronize(c->stream));
    }
    return RMX_OK;
}

int rmx_solve_batch(rmx_ctx* c, const double* buoy_xyz, int n_buoys, const int32_t* pairs, int n_pairs,
                    const int32_t* lag_int, const float* lag_frac, const float* weight, double sample_rate_hz,
                    int n_windows, int max_iter, double* pos, double* cost, int32_t* iters, unsigned flags) {
    return solve_request(c, buoy_xyz, n_buoys, pairs, n_pairs, lag_int, lag_frac, weight, sample_rate_hz, n_windows, max_iter, pos, cost,
                         iters, flags, nullptr);
}

// rmx_solve_batch with the plane and the outputs at the fix: k_solve itself (plane == NULL) or k_solve_plane, then k_solve_fix
// at the position either wrote, on the ctx stream.
int rmx_solve_batch_fix(rmx_ctx* c, const double* buoy_xyz, int n_buoys, const int32_t* pairs, int n_pairs,
                        const int32_t* lag_int, const float* lag_frac, const float* weight, double sample_rate_hz,
                        const double* plane, int n_windows, int max_iter, double* pos, double* cost, int32_t* iters,
                        double* info, double* cov, double* resid, unsigned flags) {
    const SolveFixArgs fx{plane, info, cov, resid};
    return solve_request(c, buoy_xyz, n_buoys, pairs, n_pairs, lag_int, lag_frac, weight, sample_rate_hz, n_windows, max_iter, pos, cost,
                         iters, flags, &fx);
}

int rmx_detect_batch(rmx_ctx* c, const void* iq, int n_windows, int n_samples, float threshold_db, int distance,
                     double dc_exclude_bins, float min_confidence, int max_peaks, int32_t* count, int32_t* bin,
                     float* power_db, float* snr_db, float* confidence, float* noise_floor_db, unsigned flags) {
    if (!c) return RMX_E_INVAL;
    if (!iq || !count || !bin || !power_db || !snr_db || !confidence || !noise_floor_db)
        return fail(c, RMX_E_INVAL, "NULL buffer");
    int logn = 0;
    while ((1 << logn) < n_samples) ++logn;
    if (n_samples < 16 || n_samples > 16384 || (1 << logn) != n_samples)
        return fail(c, RMX_E_INVAL, "n_samples %d is not a power of two in 16..16384", n_samples);
    if (n_windows < 0 || distance < 1 || max_peaks < 1)
        return fail(c, RMX_E_INVAL, "n_windows %d, distance %d, max_peaks %d", n_windows, distance, max_peaks);
    if (n_windows == 0) return RMX_OK;
    RMX_HIP(c, hipSetDevice(c->device));
    const int N = n_samples;
    if (!c->dt_tw.holds(logn)) {
        std::vector<float2> t;
        rmx::gen::make_row_table(t, N);
        RMX_MEM(c->dt_tw.refill(logn, t));
        int rc_l = allow_lds(c, rmx::gen::kDetFftAllowBytes, det::d_fft_db<false>, det::d_fft_db<true>);
        if (rc_l == RMX_OK) rc_l = allow_lds(c, rmx::gen::kDetPeaksAllowBytes, det::d_peaks);
        if (rc_l != RMX_OK) return rc_l;
    }
    const bool in_dev = flags & RMX_IN_DEVICE, out_dev = flags & RMX_OUT_DEVICE, u8 = flags & RMX_IN_U8;
    RMX_MEM(c->dt_pdb.reserve((size_t)n_windows * N));
    int rc = RMX_OK;
    const void* d_iq = iq;
    if (!in_dev) {
        const size_t nb = (size_t)n_windows * N * (u8 ? 2 : 8);
        RMX_MEM(c->dt_in.reserve(nb));
        RMX_HIP(c, hipMemcpyAsync(c->dt_in, iq, nb, hipMemcpyHostToDevice, c->stream));
        d_iq = c->dt_in;
    }
    int *d_count = count, *d_bin = bin;
    float *d_pw = power_db, *d_snr = snr_db, *d_conf = confidence, *d_floor = noise_floor_db;
    const size_t per = (size_t)n_windows * max_peaks;
    if (!out_dev) {
        RMX_MEM(c->dt_out.reserve(per * 16 + (size_t)n_windows * 8));
        char* b = c->dt_out;
        d_bin = (int*)b; d_pw = (float*)(b + per * 4); d_snr = (float*)(b + per * 8); d_conf = (float*)(b + per * 12);
        d_count = (int*)(b + per * 16); d_floor = (float*)(b + per * 16 + (size_t)n_windows * 4);
    }
    const int fthr = rmx::gen::det_fft_threads(N);
    rc = with_u8(u8, [&](auto U) {
        return launch(c, kTkNone, det::d_fft_db<decltype(U)::value>, dim3(n_windows), dim3(fthr), (size_t)rmx::gen::det_fft_layout(N).bytes, d_iq, c->dt_pdb,
                      c->dt_tw, logn);
    });
    if (rc != RMX_OK) return rc;
    const int pthr = rmx::gen::det_peaks_threads(N);
    const size_t plds = (size_t)rmx::gen::det_peaks_layout(N, pthr).bytes;
    // a distance >= N keeps the single highest candidate, as N does: clamped, so that the kernel's neighbour span
    // 2 (distance - 1) + 1 stays in int range and each candidate scans at most 2 N - 1 bins
    const int dist = distance < N ? distance : N;
    rc = launch(c, kTkNone, det::d_peaks, dim3(n_windows), dim3(pthr), plds, c->dt_pdb, logn, threshold_db, dist, dc_exclude_bins,
                min_confidence, max_peaks, d_count, d_bin, d_pw, d_snr, d_conf, d_floor);
    if (rc != RMX_OK) return rc;
    if (!out_dev) {
        RMX_HIP(c, hipMemcpyAsync(bin, d_bin, per * 4, hipMemcpyDeviceToHost, c->stream));
        RMX_HIP(c, hipMemcpyAsync(power_db, d_pw, per * 4, hipMemcpyDeviceToHost, c->stream));
        RMX_HIP(c, hipMemcpyAsync(snr_db, d_snr, per * 4, hipMemcpyDeviceToHost, c->stream));
        RMX_HIP(c, hipMemcpyAsync(confidence, d_conf, per * 4, hipMemcpyDeviceToHost, c->stream));
        RMX_HIP(c, hipMemcpyAsync(count, d_count, (size_t)n_windows * 4, hipMemcpyDeviceToHost, c->stream));
        RMX_HIP(c, hipMemcpyAsync(noise_floor_db, d_floor, (size_t)n_windows * 4, hipMemcpyDeviceToHost, c->stream));
        RMX_HIP(c, hipStreamSynchronize(c->stream));
    }
    return RMX_OK;
}

int rmx_synchronize(rmx_ctx* c) {
    if (!c) return RMX_E_INVAL;
    RMX_HIP(c, hipSetDevice(c->device));
    RMX_HIP(c, hipStreamSynchronize(c->stream));
    return RMX_OK;
}

int rmx_last_timing(rmx_ctx* c, float* fwd_ms, int* fwd_launches, float* pair_ms, int* pair_launches) {
    if (!c) return RMX_E_INVAL;
    RMX_HIP(c, hipSetDevice(c->device));
    RMX_HIP(c, hipStreamSynchronize(c->stream));
    float tf = 0, tp = 0;
    int nf = 0, np = 0;
    for (size_t k = 0; k < c->ev_kind.size(); ++k) {
        float ms = 0;
        RMX_HIP(c, hipEventElapsedTime(&ms, c->ev[2 * k], c->ev[2 * k + 1]));
        if (c->ev_kind[k] == rmx::kTkFwd4096) { tf += ms; ++nf; }
        else if (c->ev_kind[k] == rmx::kTkPair4096) { tp += ms; ++np; }
    }
    if (fwd_ms) *fwd_ms = tf;
    if (fwd_launches) *fwd_launches = nf;
    if (pair_ms) *pair_ms = tp;
    if (pair_launches) *pair_launches = np;
    return RMX_OK;
}

int rmx_last_timing_kind(rmx_ctx* c, int kind, const char** name, float* ms, int* launches) {
    if (!c) return RMX_E_INVAL;
    if (kind < 0 || kind >= rmx::kTkCount) return RMX_E_INVAL;   // (no error text: callers enumerate kinds until this)
    RMX_HIP(c, hipSetDevice(c->device));
    RMX_HIP(c, hipStreamSynchronize(c->stream));
    float t = 0;
    int n = 0;
    for (size_t k = 0; k < c->ev_kind.size(); ++k) {
        if (c->ev_kind[k] != kind) continue;
        float one = 0;
        RMX_HIP(c, hipEventElapsedTime(&one, c->ev[2 * k], c->ev[2 * k + 1]));
        t += one;
        ++n;
    }
    if (name) *name = rmx::kTimeKindName[kind];
    if (ms) *ms = t;
    if (launches) *launches = n;
    return RMX_OK;
}

#ifndef RMX_SOURCE_DIGEST
#define RMX_SOURCE_DIGEST "unknown"
#endif
// (the marker in front of the digest lets __graft_entry__._stale() read it out of the file without loading the library)
const char* rmx_build_info(void) { return "RMX_BUILD_INFO source_digest=" RMX_SOURCE_DIGEST " arch=gfx950"; }

size_t rmx_scratch_bytes(const rmx_ctx* c) { return c ? c->mem.ledger : 0; }

}  // extern "C"
