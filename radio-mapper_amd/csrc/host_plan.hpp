// host_plan.hpp -- the host-only logic of the C ABI: kernel-selection options, argument checks, the pair plan and the
// chunk arithmetic.  No HIP in here: rmx_hip.hip includes it, and tests/host/test_host_plan.cpp compiles it with
// g++ -fsanitize=address,undefined (tests/test_host_plan_sanitized.py), which is the sanitizer target SURVEY.md
// section 5 asks for on the CPU side of the boundary.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace rmx {

// one pair of the plan, in the order results are written: run = pairs left in this anchor run (same i), this one included
struct PairItem {
    int i, j, out, run;
};

namespace host {

// ---- kernel-selection options ------------------------------------------------------------------------------------
// Process-wide defaults that rmx_create() copies into the new ctx (a ctx never sees later changes: the kernels, block
// sizes and LDS sizes it derived from them at creation stay consistent).  Set through rmx_set_default_option(); the
// library itself never reads the environment.  They exist for tests and A/B measurements (tools/README.md lists them).
struct OptionSpec {
    const char* key;
    long lo, hi;
    const char* what;
};
inline const std::vector<OptionSpec>& option_specs() {
    static const std::vector<OptionSpec> s = {
        {"stag", 0, 5, "N = 4096 fused kernel: which waves run the two halves between barriers in the opposite order (0 nobody: the default; 1 SIMDs 1 and 3, 2 odd waves, 3 the second wave of every SIMD, 4 one wave of every SIMD, 5 everybody); k_win8 of the experiments build: default 1"},
        {"ncus", 1, 4096, "persistent workgroups of the fused N = 4096 kernel (default: one per CU)"},
        {"chunk_windows", 1, 1 << 20, "windows per chunk of the unfused N = 4096 path"},
        {"small4096", 0, 1, "0: N = 4096 through the fused kernel however few the windows (default 1: few windows through the per-transform kernels)"},
        {"generic4096", 0, 1, "1: N = 4096 through the generic whole-window kernels instead of k_win"},
        {"small_maxl", 256, 16384, "largest zero-padded length that runs as one LDS transform per workgroup (default 8192)"},
        {"logl1", 4, 10, "four-step: log2 of the column length"},
        {"wfused", 0, 1, "0: never g_win_fused (<= 4 buoys, N = 256 ... 2048)"},
        {"wscr", 0, 2, "g_win_scr: 0 never, 2 also for batches that do not fill the chip"},
        {"wscr14", 0, 1, "0: N = 8192 with 1024 threads x one butterfly instead of 512 x two"},
        {"wscr_per_cu", 1, 8, "persistent g_win_scr workgroups per CU"},
        {"rows_anchor", 0, 64, "four-step inverse rows: 0 never g_rows_anchor, n = from n buoys on (default 6)"},
        {"fused", 0, 2, "four-step, <= 4 buoys: 0 always the two-kernel row passes, 2 g_rows_fused for any batch size"},
        {"fused_def", 0, 1, "0: the run-time pair loop of g_rows_fused also for the default plan"},
        {"gen_chunk", 1, 4096, "generic path: at most n windows per chunk of kernel launches"},
        {"rows_tpr", 1, 1024, "four-step: threads per row (selects the run-time-length row kernels)"},
        {"cols_threads", 64, 1024, "four-step: threads per column tile"},
        {"col_logt", 3, 5, "four-step: log2 columns per tile"},
        {"kwin16k", 0, 2, "N = 16384: 1 (default) k16_fwd + k16_pairs (four quarter transforms on the fused N = 4096 network) unless wscr = 2, 2 always, 0 g_win_eo15 / the four-step kernels"},
        {"k16_min_windows", 1, 1 << 30, "kwin16k = 1: smallest batch that takes k16_fwd / k16_pairs (default: 100 / (buoys + pairs), rounded up)"},
        {"kwin8k", 0, 2, "N = 8192, batches that fill the chip: 1 (default) k_win8kl (the bin-parity halves on the fused N = 4096 network, one anchor half in LDS), 0 g_win_scr14, 2 k_win8k (-DRMX_EXPERIMENTS builds only)"},
#ifdef RMX_EXPERIMENTS
        {"pk", 0, 1, "1: k_winp (packed fp32 build of the fused kernel; -DRMX_EXPERIMENTS builds only)"},
        {"win8", 0, 1, "1: k_win8 (8 points x 1024 threads; -DRMX_EXPERIMENTS builds only)"},
#endif
    };
    return s;
}

struct Knobs {
    std::map<std::string, long> v;
    bool get(const char* key, long* out) const {
        auto it = v.find(key);
        if (it == v.end()) return false;
        *out = it->second;
        return true;
    }
    long get_or(const char* key, long dflt) const {
        long x;
        return get(key, &x) ? x : dflt;
    }
};
inline std::mutex& knob_mutex() { static std::mutex m; return m; }
inline Knobs& default_knobs() { static Knobs k; return k; }

// 0, or -1 with *err set (unknown key / value out of range).  value == LONG_MIN removes the key.
inline int set_default_option(const char* key, long value, std::string* err) {
    if (!key) { if (err) *err = "NULL key"; return -1; }
    for (const OptionSpec& s : option_specs()) {
        if (std::strcmp(s.key, key) != 0) continue;
        std::lock_guard<std::mutex> g(knob_mutex());
        if (value == LONG_MIN) { default_knobs().v.erase(key); return 0; }
        if (value < s.lo || value > s.hi) {
            if (err) { char b[160]; std::snprintf(b, sizeof b, "option '%s': %ld not in %ld..%ld", key, value, s.lo, s.hi); *err = b; }
            return -1;
        }
        default_knobs().v[key] = value;
        return 0;
    }
    if (err) *err = std::string("unknown option '") + key + "'";
    return -1;
}
inline void clear_default_options() {
    std::lock_guard<std::mutex> g(knob_mutex());
    default_knobs().v.clear();
}
inline Knobs snapshot_default_options() {
    std::lock_guard<std::mutex> g(knob_mutex());
    return default_knobs();
}

// ---- argument checks ---------------------------------------------------------------------------------------------
inline bool is_pow2(long n) { return n > 0 && (n & (n - 1)) == 0; }

// rmx_create: 0 or -1 with *err
inline int check_create_args(int n_buoys, int n_samples, int max_windows, std::string* err) {
    char b[160];
    if (n_buoys < 2 || n_buoys > 4096) { std::snprintf(b, sizeof b, "n_buoys %d not in 2..4096", n_buoys); *err = b; return -1; }
    if (!is_pow2(n_samples) || n_samples < 16 || n_samples > (1 << 22)) {
        std::snprintf(b, sizeof b, "n_samples %d must be a power of two in 16..4194304", n_samples); *err = b; return -1;
    }
    if (max_windows < 1) { std::snprintf(b, sizeof b, "max_windows %d < 1", max_windows); *err = b; return -1; }
    return 0;
}

// one [lo, hi] row of a lag_bounds array (rmx_xcorr_batch_bounded): an interval inside [-(N-1), N-1]?  *full: all of it
inline bool lag_interval_ok(int lo, int hi, int n_samples, bool* full) {
    const int nm1 = n_samples - 1;
    if (lo < -nm1 || hi > nm1 || lo > hi) return false;
    *full = lo == -nm1 && hi == nm1;
    return true;
}

// one band [lo, hi] in cycles per sample (rmx_xcorr_batch_weighted) -> the signed bins s in [-N, N-1] of the 2N-point
// transform with lo <= s / 2N <= hi (exact: 2N is a power of two); hi = 0.5 is bin N, which -N stands for: clamped to N-1
enum BandCheck { kBandOk = 0, kBandNoInterval = 1, kBandNoBin = 2 };   // not an interval inside [-0.5, 0.5] / no bin kept
inline BandCheck band_to_bins(double lo, double hi, int n_samples, int32_t* s_lo, int32_t* s_hi) {
    if (!std::isfinite(lo) || !std::isfinite(hi) || lo < -0.5 || hi > 0.5 || lo > hi) return kBandNoInterval;
    const long N = n_samples, L = 2L * N;
    const long a = (long)std::ceil(lo * (double)L);
    long b = (long)std::floor(hi * (double)L);
    if (b > N - 1) b = N - 1;
    if (a > b) return kBandNoBin;
    *s_lo = (int32_t)a;
    *s_hi = (int32_t)b;
    return kBandOk;
}

// ---- the pair plan ------------------------------------------------------------------------------------------------
struct PairPlan {
    std::vector<int32_t> pairs;     // [P][2]
    std::vector<PairItem> items;    // [P]
    std::vector<int> part_begin;    // [n_parts + 1]
    int n_parts = 0;
    bool all_pairs = false;         // the default list: all i < j in nested-loop order (tdoa_processor.py:156-157)
};

// is this the default list (pairs == nullptr: n_pairs alone says)?  Reads nothing when the count is not B(B-1)/2.
inline bool is_default_list(int n_buoys, const int32_t* pairs, int n_pairs) {
    if (n_pairs != (long)n_buoys * (n_buoys - 1) / 2) return false;
    int q = 0;
    for (int i = 0; pairs && i < n_buoys; ++i)
        for (int j = i + 1; j < n_buoys; ++j, ++q)
            if (pairs[2 * q] != i || pairs[2 * q + 1] != j) return false;
    return true;
}

// every index of a caller's list names a buoy (pairs == nullptr: the default list, nothing to look at).  0, or -1 with *err.
inline int check_pair_list(int n_buoys, const int32_t* pairs, int n_pairs, std::string* err) {
    for (int q = 0; pairs && q < n_pairs; ++q) {
        const int i = pairs[2 * q], j = pairs[2 * q + 1];
        if (i < 0 || j < 0 || i >= n_buoys || j >= n_buoys) {
            char b[200];
            std::snprintf(b, sizeof b, "pair %d = (%d,%d) out of range for %d buoys", q, i, j, n_buoys);
            *err = b;
            return -1;
        }
    }
    return 0;
}

// pairs == nullptr: the default list (n_pairs must then be P = B(B-1)/2).  0, or -1 with *err.
inline int make_pair_plan(int n_buoys, const int32_t* pairs, int n_pairs, int pairs_per_block, PairPlan* out, std::string* err) {
    char b[200];
    const long all = (long)n_buoys * (n_buoys - 1) / 2;
    if (n_pairs < 0) { std::snprintf(b, sizeof b, "n_pairs %d < 0", n_pairs); *err = b; return -1; }
    if (check_pair_list(n_buoys, pairs, n_pairs, err) != 0) return -1;
    std::vector<int32_t> pl;
    if (pairs) {
        pl.assign(pairs, pairs + 2 * (size_t)n_pairs);
    } else {
        if (n_pairs != all) { std::snprintf(b, sizeof b, "pairs == NULL needs n_pairs == %ld, got %d", all, n_pairs); *err = b; return -1; }
        pl.reserve(2 * (size_t)all);
        for (int i = 0; i < n_buoys; ++i)
            for (int j = i + 1; j < n_buoys; ++j) { pl.push_back(i); pl.push_back(j); }
    }
    out->items.resize(n_pairs);
    for (int q = 0; q < n_pairs; ++q) out->items[q] = PairItem{pl[2 * q], pl[2 * q + 1], q, 1};
    for (int q = n_pairs - 2; q >= 0; --q)
        if (out->items[q].i == out->items[q + 1].i) out->items[q].run = out->items[q + 1].run + 1;
    const int ppb = pairs_per_block > 0 ? pairs_per_block : 7;
    const int n_parts = n_pairs > 0 ? (n_pairs + ppb - 1) / ppb : 0;
    out->part_begin.assign(n_parts + 1, 0);
    for (int k = 0; k <= n_parts && n_parts > 0; ++k) out->part_begin[k] = (int)((long)k * n_pairs / n_parts);
    out->n_parts = n_parts;
    out->all_pairs = is_default_list(n_buoys, pl.data(), n_pairs);
    out->pairs.swap(pl);
    return 0;
}

// ---- k_win, phase 2: the order of a window's pairs among buoys 1 .. B-1 ---------------------------------------------
// Phase 1 of the fused kernel (anchor 0) leaves X_{B-1} in register array 1 (sb) and X_1 .. X_{B-2} in the scratch.
// The remaining pairs are walked so that every pair shares one buoy with the pair before it: the shared spectrum stays
// in its register array, and each step requests ONE spectrum, into the array whose buoy the next step drops.
struct TrailStep {
    int i, j;       // the pair, i < j: the kernel computes X_j conj(X_i)
    int out_idx;    // i*B - i(i+1)/2 + (j-i-1)
    int xi_arr;     // register array (0 = sa, 1 = sb) that holds X_i; X_j is in the other one
    int load_arr;   // array that the request issued DURING this step overwrites: the one whose buoy the next step drops
    int load_idx;   // the spectrum that request loads (an operand of the next step); -1 behind the last step
    int reload;     // 1: the next step shares no buoy with this one, load2 goes into the other array as well
    int load2;      // -1 unless reload
};
struct PairTrail {
    int n_buoys = 0;
    int first_load = -1;   // requested by the last pair of phase 1 into array 0: the first step's other operand (-1: no step)
    std::vector<TrailStep> steps;
    int loads = 0;         // spectrum requests issued by the steps: one per step but the last, two where `reload`;
                           // with first_load that is loads + 1 spectrum loads per window (21 at B = 8)
    int reloads = 0, min_reloads = 0;   // steps that reload both arrays, and the fewest the order's construction needs
    int sim_hits2 = 0, sim_hits3 = 0;   // of first_load + loads: hits in an LRU of two / three spectra (trail_sim_hits)
};

inline int trail_out_idx(int B, int i, int j) { return i * B - (i * (i + 1)) / 2 + (j - i - 1); }

// One window's spectrum traffic through an LRU of `cap` spectra: the stores of X_1 .. X_{B-2} (write-allocate), then
// first_load and every step's requests in order.  Returns the requests that hit.  (A model for the notes: two spectra are a
// workgroup's share of its XCD's L2; LABNOTES R10.1 sets it against the measured counters.)
inline int trail_sim_hits(const PairTrail& t, int cap) {
    std::vector<int> lru;   // most recent first
    auto touch = [&](int b) -> bool {
        bool hit = false;
        for (size_t k = 0; k < lru.size(); ++k)
            if (lru[k] == b) { lru.erase(lru.begin() + (long)k); hit = true; break; }
        lru.insert(lru.begin(), b);
        if ((int)lru.size() > cap) lru.pop_back();
        return hit;
    };
    int hits = 0;
    for (int b = 1; b + 1 < t.n_buoys; ++b) touch(b);
    if (t.first_load >= 0) hits += touch(t.first_load);
    for (const TrailStep& s : t.steps) {
        if (s.load_idx >= 0) hits += touch(s.load_idx);
        if (s.reload) hits += touch(s.load2);
    }
    return hits;
}

// steps from a list of pairs in walking order (the first one holds B-1, resident in array 1): a pair that shares a buoy
// with the one before it keeps that buoy where it is; one that shares none is a reload of both arrays
inline void trail_from_pairs(int B, const std::vector<std::pair<int, int>>& pairs, PairTrail* t) {
    t->n_buoys = B;
    t->steps.clear();
    t->loads = t->reloads = 0;
    t->first_load = -1;
    if (pairs.empty()) return;
    t->first_load = pairs[0].first == B - 1 ? pairs[0].second : pairs[0].first;
    int arr_of[2] = {t->first_load, B - 1};
    for (size_t k = 0; k < pairs.size(); ++k) {
        const int a = pairs[k].first, b = pairs[k].second;
        TrailStep s{};
        s.i = a < b ? a : b;
        s.j = a < b ? b : a;
        s.out_idx = trail_out_idx(B, s.i, s.j);
        s.xi_arr = arr_of[0] == s.i ? 0 : 1;
        s.load_arr = 0; s.load_idx = -1; s.reload = 0; s.load2 = -1;
        if (k + 1 < pairs.size()) {
            const int c = pairs[k + 1].first, d = pairs[k + 1].second;
            const bool keep_c = c == a || c == b, keep_d = d == a || d == b;
            if (keep_c == keep_d) {          // no shared buoy (or the same pair again, which the planner never emits)
                s.reload = 1;
                s.load_arr = 0; s.load_idx = c < d ? c : d; s.load2 = c < d ? d : c;
                arr_of[0] = s.load_idx; arr_of[1] = s.load2;
                t->loads += 2;
                ++t->reloads;
            } else {
                const int keep = keep_c ? c : d;
                s.load_arr = arr_of[0] == keep ? 1 : 0;
                s.load_idx = keep_c ? d : c;
                arr_of[s.load_arr] = s.load_idx;
                ++t->loads;
            }
        }
        t->steps.push_back(s);
    }
    t->sim_hits2 = trail_sim_hits(*t, 2);
    t->sim_hits3 = trail_sim_hits(*t, 3);
}

// THE order k_win walks: runs that hand the anchor over.  A run (a, r1), (a, r2), ... keeps the anchor a where it is and
// streams the r, and its last pair (a, r_last) is followed by (r_last, r'): the spectrum streamed last stays in ITS array
// as the next anchor, and the stream moves to the array the old anchor leaves.  Every buoy becomes anchor once, with the
// buoys that have not been one as its stream, so every pair appears once, no step reloads both arrays whatever the parity
// of B (min_reloads = 0), and no anchor is ever loaded.  Each run streams the previous run's order backwards (less its
// last buoy, the new anchor), so its first request is the spectrum requested second to last.  The first run is anchored
// at B-1 (resident behind phase 1) and streams B-2 first, which phase 1 stored last but one.  Anchors alternate between
// the highest and the lowest buoy left, streamed from the far end, which puts X_i into array 0 at every step.
// (An Eulerian trail of the complete graph on buoys 1 .. B-1 -- one shared buoy per step, changing at every step -- was
// built and measured first: odd B forces (B-1)/2 - 1 reloads, and no spectrum comes back before two others have passed;
// LABNOTES R10.1 has its table and counters.)
inline PairTrail plan_pair_trail(int B) {
    PairTrail t;
    t.n_buoys = B;
    const int n = B - 1;
    std::vector<std::pair<int, int>> pairs;
    std::vector<int> order;
    for (int r = n - 1; r >= 1; --r) order.push_back(r);
    int anchor = n;
    while (!order.empty()) {
        for (int r : order) pairs.push_back({anchor, r});
        anchor = order.back();
        order.pop_back();
        for (size_t a = 0, b = order.size(); a + 1 < b; ++a, --b) { const int x = order[a]; order[a] = order[b - 1]; order[b - 1] = x; }
    }
    trail_from_pairs(B, pairs, &t);
    t.min_reloads = 0;
    return t;
}

// what k_win's phase 2 can walk: X_i in array 0 at every step and never a reload of both arrays (it has one copy of h1
// per request target, none per role).  rmx_create refuses a table that is anything else.
// And no request for X_{B-1}: it stays in array 1 behind phase 1 and is the one spectrum phase 1 does not store, so its
// slot of the scratch holds nothing of this window.
inline bool trail_kernel_ok(const PairTrail& t) {
    const int last = t.n_buoys - 1;
    if (!t.steps.empty() && t.first_load == last) return false;
    for (const TrailStep& s : t.steps)
        if (s.xi_arr != 0 || s.reload != 0 || s.load_idx == last) return false;
    return true;
}

// The kernel's copy: (pairs + 1) entries of four ints {out_idx, load_arr, load_idx, 0} (16 bytes: one scalar load).  Entry
// 0 is the last pair of phase 1, (0, B-1), whose request is first_load into array 0; entry k + 1 is step k.  Where a step
// requests nothing, the entry names a spectrum that phase 1 stored (the kernel requests unconditionally into dead
// registers): buoy 1, never B-1, whose slot nobody writes.  (B = 2 stores nothing and requests nothing: entry 0 names 0.)
// Empty for a table the kernel cannot walk (trail_kernel_ok).
inline std::vector<int32_t> encode_pair_trail(const PairTrail& t) {
    std::vector<int32_t> e;
    if (!trail_kernel_ok(t)) return e;
    const int B = t.n_buoys;
    e.reserve(4 * (t.steps.size() + 1));
    const int some = B > 2 ? 1 : 0;
    e.insert(e.end(), {trail_out_idx(B, 0, B - 1), 0, t.first_load >= 0 ? t.first_load : some, 0});
    for (const TrailStep& s : t.steps)
        e.insert(e.end(), {s.out_idx, s.load_arr, s.load_idx >= 0 ? s.load_idx : some, 0});
    return e;
}

// ---- chunk arithmetic of the generic path ----------------------------------------------------------------------------
// windows per chunk of kernel launches: spectra (B*L) + products (P*L), 8 bytes each, under `budget_bytes` (32 GiB of
// the 288: cfg2's 64 windows of 2^20 samples are one chunk of 6.4 GB), at most 4096 and at most max_windows
inline long generic_chunk_windows(int n_buoys, long L, int max_windows, long budget_bytes, long cap) {
    const long all_pairs = (long)n_buoys * (n_buoys - 1) / 2;
    const long per_win = (long)(n_buoys + all_pairs) * L * 8;
    long chunk = per_win > 0 ? budget_bytes / per_win : 1;
    if (chunk < 1) chunk = 1;
    if (chunk > max_windows) chunk = max_windows;
    if (chunk > 4096) chunk = 4096;
    if (cap >= 1 && cap < chunk) chunk = cap;
    return chunk;
}

// ---- several bands per window (rmx_xcorr_batch_bands): the buffer arithmetic ---------------------------------------------
// A banded call correlates every real window under n_bands bands: a chunk of `chunk` real windows is chunk * n_bands
// VIRTUAL windows to the pair kernels, and every per-slot buffer holds chunk * n_bands * n_pairs slots instead of
// chunk * n_pairs -- the four-step products, tile records and halo rows, and (per call) the three outputs.  plan_bands is
// the one place that arithmetic lives: it SHRINKS the chunk until a chunk's virtual windows are at most `max_vwindows`
// (the cap generic_chunk_windows puts on a chunk's windows) and, on the four-step route, its spectra and products fit
// `budget_bytes`, and it STATES the bytes each buffer must then hold; the launch code allocates exactly those and launches
// at most `chunk` windows at a time (a launch sized by one rule over a buffer sized by another ran past it).
// n_bands = 1 leaves the chunk as it is.
constexpr long kGenericBudgetBytes = 32L << 30;   // spectra + products of a chunk (generic_chunk_windows)
constexpr long kGenericMaxChunk = 4096;
// The most grid rows (second grid dimension) the library gives a launch.  Not a limit of the runtime: HIP on gfx950 took
// g_cols_inv with 67 200 rows (16 buoys x 560 windows of 8192 samples, PHAT) and every slot came out right (LABNOTES R19);
// it is the bound the library states for itself, so that no grid is larger than the ones tests/test_gpu_large_batches.py
// runs on both sides of it, and every planner below cuts its chunks to it.
constexpr long kMaxGridY = 65535;
// grid rows of a chunk's g_cols_inv launch: one per output slot -- (window, band, pair), or (group, band, pair) of an
// integrated call, whose chunk holds whole groups of `integ` windows.  generic_pairs launches exactly this many.
inline long cols_inv_grid_rows(long chunk, int n_bands, int n_pairs, int integ) {
    const long nb = n_bands > 1 ? n_bands : 1, np = n_pairs > 0 ? n_pairs : 0, K = integ > 1 ? integ : 1;
    return chunk * nb * np / K;
}
// `chunk` windows cut, in whole groups of `integ`, until that launch has at most kMaxGridY rows.  One group stays one
// chunk even where its own n_bands * n_pairs slots are more (a pair list beyond 65535 pairs): nothing smaller can be
// launched, and a group is never split.
inline long cap_chunk_grid_rows(long chunk, int n_bands, int n_pairs, int integ) {
    const long K = integ > 1 ? integ : 1;
    const long per_group = cols_inv_grid_rows(K, n_bands, n_pairs, (int)K);
    if (per_group <= 0 || cols_inv_grid_rows(chunk, n_bands, n_pairs, integ) <= kMaxGridY) return chunk;
    const long groups = kMaxGridY / per_group > 1 ? kMaxGridY / per_group : 1;
    return groups * K < chunk ? groups * K : chunk;
}
struct BandsPlan {
    long chunk = 0;          // real windows per chunk, >= 1
    long vwindows = 0;       // virtual windows of a full chunk: chunk * n_bands
    long slots = 0;          // slots of a full chunk: vwindows * n_pairs
    size_t prod_bytes = 0;   // four-step: slots * L * 8 (g_prod); 0 on the other routes
    size_t rec_bytes = 0;    // four-step: slots * col_tiles * rec_size (g_rec)
    size_t halo_bytes = 0;   // four-step: slots * col_tiles * 2 * 4 << logL1 (g_halo)
    size_t out_elems = 0;    // elements of each of the call's three outputs: n_windows * n_bands * n_pairs
};
inline BandsPlan plan_bands(long chunk, long n_windows, int n_bands, int n_buoys, int n_pairs, long L, bool four_step, long col_tiles,
                            int logL1, size_t rec_size, long budget_bytes = kGenericBudgetBytes, long max_vwindows = kGenericMaxChunk) {
    BandsPlan b;
    const long nb = n_bands > 0 ? n_bands : 1, np = n_pairs > 0 ? n_pairs : 0;
    if (chunk < 1) chunk = 1;
    if (nb > 1) {
        if (chunk * nb > max_vwindows) chunk = max_vwindows / nb;
        if (four_step) {
            const long per_win = ((long)n_buoys + nb * np) * L * 8;
            if (per_win > 0 && chunk > budget_bytes / per_win) chunk = budget_bytes / per_win;
            chunk = cap_chunk_grid_rows(chunk, (int)nb, (int)np, 1);   // g_cols_inv: one grid row per slot
        }
        if (chunk < 1) chunk = 1;
    }
    b.chunk = chunk;
    b.vwindows = chunk * nb;
    b.slots = b.vwindows * np;
    if (four_step) {
        b.prod_bytes = (size_t)b.slots * (size_t)L * 8;
        b.rec_bytes = (size_t)b.slots * (size_t)col_tiles * rec_size;
        b.halo_bytes = ((size_t)b.slots * (size_t)col_tiles * 2 * sizeof(float)) << logL1;
    }
    b.out_elems = (size_t)(n_windows > 0 ? n_windows : 0) * (size_t)nb * (size_t)np;
    return b;
}

// ---- N = 4096: fused kernel or per-transform kernels, and how many pairs per workgroup -----------------------------
// Estimated microseconds, fitted to tools/exp_small4096.py on MI355X: 2.6 per transform of the
// fused kernel (one workgroup per window, a round = one window on every CU); 3.5 per round of forward workgroups (two per
// CU); 4.0 per pair workgroup + 3.3 per pair in it (one per CU); a round that fills the chip runs up to 45 % slower than
// a lone workgroup, less so when many rounds follow each other out of step.
inline double fused_cost4096(int n_cus, int n_buoys, int n_pairs, long n_windows) {
    const long cus = n_cus > 0 ? n_cus : 1;
    return (double)((n_windows + cus - 1) / cus) * (n_buoys + n_pairs) * 2.6 + 3.0;
}
// the per-transform estimate and the pairs per workgroup (1 ... 7, or `fixed_ppb` when the caller set them) that minimise it
inline double split_cost4096(int n_cus, int n_buoys, int n_pairs, long n_windows, int fixed_ppb, int* ppb) {
    const long cus = n_cus > 0 ? n_cus : 1;
    auto rounds = [](long blocks, long per_round) { return (double)((blocks + per_round - 1) / per_round); };
    const double t_fwd = rounds(n_windows * n_buoys, 2 * cus) * 3.5 + 2.0;
    double best = 1e30;
    *ppb = fixed_ppb > 0 ? fixed_ppb : 7;
    for (int q = 7; q >= 1; --q) {
        const int qq = fixed_ppb > 0 ? fixed_ppb : q;
        const long parts = n_pairs > 0 ? (n_pairs + qq - 1) / qq : 1;
        const long blocks = n_windows * parts;
        const double r = blocks > 0 ? rounds(blocks, cus) : 1.0;
        const double fill = blocks >= cus ? 1.0 : (double)blocks / (double)cus;
        const double t = (t_fwd + r * (4.0 + 3.3 * (double)((n_pairs + parts - 1) / parts))) * (1.15 + 0.3 * fill / std::sqrt(r));
        if (t < best) { best = t; *ppb = qq; }
        if (fixed_ppb > 0) break;
    }
    return best;
}

// ---- the route of one correlation call ---------------------------------------------------------------------------------
// plan_route is the ONE place where a call's kernels are chosen; the launch code executes the plan.
enum Route {
    kRouteKWin,        // N = 4096: k_win, forward + pairs in one workgroup per window (a chunk's partial round: route_wtail4096)
    kRoutePer4096,     // N = 4096: k_fwd + k_pair_res / k_pair_str per chunk
    kRouteK16,         // N = 16384: k16_fwd + k16_pairs per chunk of ws_grid windows
    kRouteKWin8,       // N = 8192: k_win8kl (k_win8k in an experiments build), the batch's partial round through the per-transform kernels
    kRouteWinScr,      // g_win_scr / g_win_scr14: whole windows, spectra in a cache-resident scratch
    kRouteWinEo15,     // N = 16384: g_win_eo15, the partial round as for k_win8kl
    kRouteWinFused,    // <= 4 buoys, L <= 4096: g_win_fused, spectra in registers
    kRouteSmallL,      // L <= small_maxl: g_fwd_small + g_pair_small per chunk
    kRouteFourStep     // longer: the column and row passes per chunk (route_rows_fused: g_rows_fused does both row passes)
};
enum RouteRefusal { kRouteOk = 0, kRefuseIntegChunk, kRefuseIntegTile, kRefuseBandsChunk };   // integrate > a chunk (RoutePlan::bands_chunk > 0: after
                                                                             // the bands shrank it) / column tile too large per thread /
                                                                             // plan_caf: one window's n_bands * n_pairs slots are more than any chunk holds

// what rmx_create / generic_init (and rmx_set_option) fixed for the ctx
struct RouteCaps {
    int n_cus = 1, n_buoys = 2, logL = 13, logL1 = 0, logL2 = 0;
    bool generic = false;
    long small_maxl = 8192;
    bool fused = true, small_batch = true;   // N = 4096 ...
    int chunk_windows = 8, ppb_user = 0;     // ... ppb_user: the caller's pairs per workgroup, or 0
    int g_chunk = 1, ws_upw = 0, ws_grid = 0, k16 = 0;   // generic ...
    bool wfused = false, wscr = false, wscr_always = false, k8 = false, g_fused = false, g_fused_always = false;
    long k16_min_windows = 0;                // option k16_min_windows, or 0: 100 / (buoys + pairs), rounded up
    int max_pairs8 = 640, max_pairs16 = 640;                               // k8::kMaxPairs8, k16::kMaxPairs16
    long col_tile = 0;  int cols_threads = 1, integ_max_per_thread = 16;   // four-step column tile, its threads, kIntegMaxPerThread
};
// what the call asks
struct RouteCall {
    int n_windows = 0, n_pairs = 0;
    bool all_pairs = true, pairs_given = false;   // PairPlan::all_pairs; the caller passed a list (which may still be the default one)
    bool bounded = false, weighted = false;       // XcorrCall::bounded(), XcorrCall::weighted()
    int integ = 1;
    bool in_dev = true;
    int n_bands = 1;                              // rmx_xcorr_batch_bands: the pair kernels see n_windows * n_bands virtual windows
};
struct RoutePlan {
    Route route = kRoutePer4096;
    int ppb = 7;                 // pairs per workgroup of the N = 4096 pair kernels (unused elsewhere)
    int chunk = 0;               // windows per chunk of the per-transform routes and of k16, a multiple of integ
    int n_head = 0, n_tail = 0;  // k_win8kl / g_win_eo15: windows of the full rounds / of the partial round behind them
    int tail = 0;                // k_win: the largest partial round of any chunk that pays (the gate of route_wtail4096), or 0
    bool pipelined = false;      // k_win, host windows: the copy is cut into sub-chunks on a second stream
    RouteRefusal refused = kRouteOk;
    int bands_chunk = 0;         // banded integrated call: the chunk plan_bands allows, before it is rounded down to whole groups
                                 // (kRefuseIntegChunk with bands_chunk > 0: the bands shrank the chunk below one group)
};

constexpr int kHostSubChunk = 512;   // windows per copy/kernel step of the pipelined host-pointer path

// N = 4096, k_win: r windows through the per-transform kernels are cheaper than one more round of the fused kernel
inline bool tail_pays4096(const RouteCaps& k, int n_pairs, int r, int* q) {
    return split_cost4096(k.n_cus, k.n_buoys, n_pairs, r, k.ppb_user, q) < 0.9 * fused_cost4096(k.n_cus, k.n_buoys, n_pairs, 1);
}
// This chunk's partial round (windows [w0, w0 + wc) of the call): only behind at least one full round of this call, and
// only when the model says so for ITS size -- with the default chunk (a multiple of the CU count) that is the batch's last
// partial round; 0 <= wtail < CUs and wtail <= wc by construction
inline int route_wtail4096(const RouteCaps& k, const RoutePlan& p, int n_pairs, int w0, int wc) {
    if (!p.tail || !(w0 > 0 || wc > k.n_cus) || wc % k.n_cus == 0) return 0;
    int q_unused = 7;
    return tail_pays4096(k, n_pairs, wc % k.n_cus, &q_unused) ? wc % k.n_cus : 0;
}
// Four-step: the fused row kernel when its (window, row block) units fill the chip at least twice: below that (cfg1's single
// window: 128 workgroups) its long serial chain per unit loses to the two-kernel passes' wider grids (57 vs 47 us).  Never for
// a weighted() call: g_rows_fused keeps its spectra to itself.
inline bool route_rows_fused(const RouteCaps& k, bool weighted, int wc) {
    if (weighted || !k.generic || !k.g_fused || (1L << k.logL) <= k.small_maxl) return false;
    const long fused_blocks = (long)wc * (1L << k.logL1) / (256 / ((1 << k.logL2) >> 4));   // (256: gen::kGThreads)
    return fused_blocks >= 2L * k.n_cus || k.g_fused_always;
}

// An integrated call's chunk (plan_route and plan_caf): `chunk` windows rounded down to whole groups -- never a silent
// split of a group --, refused when that leaves none, or when the four-step column kernel would sum more per thread than it holds
inline RouteRefusal integ_chunk(const RouteCaps& k, int chunk, int integ, bool four_step, int* whole_groups) {
    *whole_groups = chunk / integ * integ;
    if (*whole_groups == 0) return kRefuseIntegChunk;
    if (integ > 1 && four_step && k.col_tile > (long)k.integ_max_per_thread * k.cols_threads) return kRefuseIntegTile;
    return kRouteOk;
}

inline RoutePlan plan_route4096(const RouteCaps& k, const RouteCall& a) {
    RoutePlan p;
    const int all_pairs = k.n_buoys * (k.n_buoys - 1) / 2, W = a.n_windows;
    auto split = [&](long w, int* q) { return split_cost4096(k.n_cus, k.n_buoys, a.n_pairs, w, k.ppb_user, q); };
    // Few windows of N = 4096: the fused kernel is one workgroup per WINDOW -- (B + P) transforms in sequence, 92 us for
    // one window of 8 buoys, 344 us for 16 buoys, whatever the rest of the chip does -- while the per-transform kernels
    // spread a window's spectra and pairs over the CUs: 13-15 us for the same single windows (tools/exp_small4096.py;
    // the crossover sits at 64 / 110 / 140 windows for 3 / 8 / 16 buoys).  This is the shape of the reference's seam:
    // one frequency group per call (tdoa_processor.py:363-377).  Both paths are costed with the model above and the
    // cheaper one runs; the same model picks the pairs per workgroup (1 ... 7) unless the caller set them.
    const bool modelled = k.fused && k.small_batch && k.n_buoys >= 3 && a.n_pairs == all_pairs;
    bool small = false;  int ppb_small = 7;
    if (modelled) small = split(W, &ppb_small) < fused_cost4096(k.n_cus, k.n_buoys, a.n_pairs, W);
    // a weighted call weights the spectra where k_fwd stores them: the per-transform kernels at every batch size, never
    // k_win (whose spectra stay inside the workgroup); an integrated call sums over windows inside k_pair_str: the same
    // kernels, with one work item per (group, pair)
    if (a.weighted) { (void)split((long)W * a.n_bands / a.integ, &ppb_small); small = true; }
    // The same arithmetic for the LAST round of a larger batch: W = k CUs + r windows cost the fused kernel k + 1 rounds
    // (300 windows of 8 buoys: two rounds, 184 us); when the model says the r windows are cheaper through the
    // per-transform kernels than a round of the fused one, they go there (after the k full rounds, on the same stream).
    // The decision is taken per CHUNK of windows (a batch-wide tail larger than the last chunk ran past the
    // chunk and past the spectrum scratch): route_wtail4096 decides for a chunk's own partial round, wc mod CUs, so it
    // never exceeds the chunk, and the scratch of min(chunk, CUs) window slots covers it.  `tail` is the gate -- the
    // largest remainder of ANY chunk that pays (every chunk but the last has chunk_windows windows; ADVICE r04: it used
    // to look at the last chunk only) -- and sizes the pair workgroups (one plan per call) for that largest partial round.
    const bool tail_ok = !small && modelled && k.n_cus > 0 && (a.in_dev || W <= kHostSubChunk);
    if (tail_ok && W > k.n_cus) {
        const long cw = k.chunk_windows;
        const int last_wc = (int)(W - ((long)(W - 1) / cw) * cw);   // windows of the last chunk
        const int r_last = last_wc % k.n_cus;
        const int r_full = (W > cw) ? (int)(cw % k.n_cus) : 0;      // every earlier chunk's remainder
        for (int r : {r_full > r_last ? r_full : r_last, r_full > r_last ? r_last : r_full}) {
            int q = 7;
            if (r != 0 && tail_pays4096(k, a.n_pairs, r, &q)) { p.tail = r; ppb_small = q; break; }
        }
    }
    if (k.ppb_user) p.ppb = k.ppb_user;
    else if (!small && !p.tail && (a.pairs_given || !k.fused)) (void)split(W, &p.ppb);   // a custom pair list (or fused = 0): the per-transform kernels anyway
    else p.ppb = (small || p.tail) ? ppb_small : 7;
    const bool fused_now = k.fused && a.all_pairs && !small;
    if (!fused_now) p.tail = 0;
    p.route = fused_now ? kRouteKWin : kRoutePer4096;
    // fused path: the host copy is cut into sub-chunks issued on a second stream, each followed by its kernel launch, so
    // that copy k+1 travels while kernel k runs; otherwise one copy up front
    p.pipelined = !a.in_dev && fused_now && W > kHostSubChunk;
    p.refused = integ_chunk(k, k.chunk_windows, a.integ, false, &p.chunk);
    return p;
}

inline RoutePlan plan_route(const RouteCaps& k, const RouteCall& a) {
    if (!k.generic) return plan_route4096(k, a);
    RoutePlan p;
    const int W = a.n_windows;
    p.n_head = W;
    // N = 16384 on k_win's network (kwin16k.hpp): fine-grained items, so no partial last round and a low minimum batch -- its
    // two launches cost about 40 us whatever the size, the four-step kernels 26 us for one window: from about 100 transforms
    // (windows x (buoys + pairs)) on it wins (tools/exp_k16_sweep.py: 3 buoys from 16 windows, 5 from 8, 8 from 1).  wscr = 2
    // (tests: "the whole-window kernel, whatever the batch") keeps g_win_eo15, as do pair lists beyond the kernel's LDS copy.
    // Weighted calls weight the spectra where the per-transform forward kernels store them: g_fwd_small up to
    // L = small_maxl, g_cols_fwd + the forward g_rows above.  The whole-window kernels (g_win_*, k_win8kl), k16_fwd and
    // g_rows_fused keep their spectra to themselves and are never taken.  Integrated calls sum over windows inside the
    // per-transform pair kernels: the same routes.
    const long k16_min = k.k16_min_windows > 0 ? k.k16_min_windows : (100 + k.n_buoys + a.n_pairs - 1) / (k.n_buoys + a.n_pairs);
    if (!a.weighted && k.k16 && k.logL == 15 && a.n_pairs <= k.max_pairs16 &&
        (k.k16 == 2 || (!k.wscr_always && W >= (int)k16_min))) { p.route = kRouteK16; p.chunk = k.ws_grid; return p; }
    // g_win_scr runs a window's B + P transforms one after the other in one workgroup: batches that leave most of the chip
    // without a workgroup are better off in the per-transform kernels (8 buoys x 8 windows of 8192: 0.32 vs 0.05 ms).
    // Measured crossovers (tools/smallw.sh): 0.43 workgroups per CU at L = 16384 (8 buoys; 0.63 with 3), 0.66 .. 0.68 below
    // (L = 32768, g_win_eo15: it wins from about 0.7 workgroups per CU on for 2 ... 16 buoys -- 0.67-0.79 x the four-step's time
    // at 256 windows, 0.85-0.94 x at 192, 0.9-1.25 x at 128: profiles/r03_weo_sweep.log)
    // (L = 16384 through k_win8kl: 242 us for anything up to one window per CU at 8 buoys, 50 us at 3, against 194 / 50 us at
    // 64 windows and 290 / 64 us at 96 through the per-transform kernels -- tools/exp_k8_small.py: from 5/16 of a workgroup per CU)
    const int upw = k.ws_upw > 0 ? k.ws_upw : 1;
    const long ws_blocks = ((long)W + upw - 1) / upw;
    // Bounded calls: of the whole-window kernels only k_win8kl has a bounded instantiation.  g_win_fused, g_win_scr,
    // g_win_scr14 and g_win_eo15 have none: a bounded call that would take one of them takes the per-transform kernels
    // instead, whose peak searches are bounded.  At the BASELINE shapes the fused kernels run either way (k_win, k_win8kl, k16_pairs).
    const bool k8_route = k.k8 && (a.all_pairs || a.n_pairs <= k.max_pairs8);
    const bool use_wscr = !a.weighted && k.wscr && (!a.bounded || k8_route) &&
                          (k.wscr_always || ws_blocks >= (k.logL == 14 ? (k.k8 ? 5L : 7L) : 11L) * k.n_cus / 16);
    if (use_wscr) {
        // k_win8kl, g_win_eo15: the batch's last, partial round (W mod grid windows behind at least one full round) costs the
        // kernel a whole round whatever its size -- k_win8kl 3.5 us per half transform: 245 us at 8 buoys, 50 at 3; g_win_eo15
        // 12.6 us: 907 us at 8 buoys --, the four-step kernels about 30 us + 0.07 us per window and spectrum-or-pair (0.14 at
        // L = 32768; tools/exp_k8_small.py: 8 buoys 104 us for 32 windows, 140 for 48; 3 buoys 43 / 47) plus four more launches.
        // The cheaper one runs, on the same stream behind the full rounds: 8 buoys x 300 windows 507 -> 444 us, x 560
        // 762 -> 710; 3 buoys never split.  Not with wscr = 2 (tests force the kernel).
        auto partial_round = [&](double us_half, double base_us, double us_item, long wg16, double margin) {
            if (k.wscr_always || k.ws_grid <= 0 || W <= k.ws_grid) return;
            const int r = W % k.ws_grid;
            const double round_us = us_half * (2.0 * k.n_buoys + 2.0 * a.n_pairs);
            const double four_us = base_us + us_item * r * (double)(k.n_buoys + a.n_pairs);
            if (r > 0 && (long)r * 16 < wg16 * k.n_cus && four_us < margin * round_us) p.n_tail = r;
        };
        p.route = k8_route ? kRouteKWin8 : k.logL == 15 ? kRouteWinEo15 : kRouteWinScr;
        if (p.route == kRouteKWin8) partial_round(3.5, 40.0, 0.07, 5, 0.7);   // (5 buoys x 300: 234 split, 228 whole)
        if (p.route == kRouteWinEo15 && k.ws_upw == 1) partial_round(12.6, 60.0, 0.14, 11, 0.85);
        p.n_head = W - p.n_tail;
        p.chunk = k.g_chunk;   // (of the partial round: plain or bounded calls only, integ = 1)
        if ((1L << k.logL) > k.small_maxl) p.chunk = (int)cap_chunk_grid_rows(p.chunk, 1, a.n_pairs, 1);   // (it runs four-step)
        return p;
    }
    if (!a.weighted && k.wfused && !a.bounded) { p.route = kRouteWinFused; return p; }
    p.route = (1L << k.logL) <= k.small_maxl ? kRouteSmallL : kRouteFourStep;
    // banded call: the chunk whose virtual windows the per-slot buffers hold (plan_bands: the sizes); banded AND integrated:
    // that chunk first, then rounded down to whole groups -- both caps hold, and no group is ever split
    const bool four_step = p.route == kRouteFourStep;
    int chunk = k.g_chunk;
    if (a.n_bands > 1) {
        chunk = (int)plan_bands(k.g_chunk, W, a.n_bands, k.n_buoys, a.n_pairs, 1L << k.logL, four_step, 0, 0, 0).chunk;
        if (a.integ > 1 && k.g_chunk >= a.integ) p.bands_chunk = chunk;
    } else if (four_step) {
        // one band: the same cap on g_cols_inv's grid rows that plan_bands puts on a banded chunk, in whole groups
        chunk = (int)cap_chunk_grid_rows(chunk, 1, a.n_pairs, a.integ);
    }
    p.refused = integ_chunk(k, chunk, a.integ, four_step, &p.chunk);
    return p;
}

// ---- the shape of one Doppler search ----------------------------------------------------------------------------------
// plan_caf is the ONE place where it is decided; caf_request in rmx_hip.hip executes the plan.
constexpr size_t kSpecBytes4096 = 64 * 1024;   // one stored N = 4096 spectrum: 8192 bins of 8 bytes
struct CafCall {
    int n_windows = 0, n_pairs = 0, n_dopplers = 1;
    int integ = 1;            // K windows per group
    bool fine = false;        // dop_frac is asked for
    bool refined = false, qualified = false;
    bool out_dev = false;     // RMX_OUT_DEVICE
    int n_bands = 1;          // rmx_caf_batch_bands: the pair kernels see n_bands virtual windows per (hypothesis, window)
};
struct CafPlan {
    bool one_launch = false;       // N = 4096: every hypothesis in ONE forward and ONE pair launch (virtual window = hypothesis x window;
                                   // n_bands > 1: (hypothesis x window) x band)
    int ppb = 7;                   // pairs per workgroup of the N = 4096 pair kernels (unused elsewhere)
    int chunk = 0;                 // windows per chunk of the per-hypothesis sweep, a multiple of integ
    RouteRefusal refused = kRouteOk;
    size_t out_elems = 0;          // elements of each output: one slot per (group, pair); n_bands > 1: per (window, band, pair)
    size_t hyp_elems = 0;          // elements of each per-hypothesis result array: [d][group][pair] in one launch, else one hypothesis'
    bool need_nb = false;          // caf_nb: k_caf_select_fd's three neighbour rows, and dop_frac of a host-pointer call behind them
    bool stage_dfrac = false;      // dop_frac is written to the ctx's block (the fourth row of caf_nb) and copied to the caller
    bool second_sweep = false;     // the hypotheses of each chunk once more, each followed by k_quality / k_refine on the slots it won
};
constexpr long kCafMaxVirtualWindows = 1L << 20;   // virtual windows of one pair launch of the Doppler search
inline CafPlan plan_caf(const RouteCaps& k, const CafCall& a) {
    CafPlan p;
    const long W = a.n_windows, D = a.n_dopplers, M = a.n_bands > 1 ? a.n_bands : 1;
    // 21 hypotheses on one frequency group: 431 -> ~60 us against three launches per hypothesis.  One chunk, at most 1 GiB
    // of de-rotated spectra (D * W * B of them whatever the bands), and virtual windows (D * W * M) that the pair kernels' grids hold
    p.one_launch = !k.generic && D > 1 && W <= k.chunk_windows && (size_t)D * W * k.n_buoys * kSpecBytes4096 <= ((size_t)1 << 30) &&
                   D * W * M < kCafMaxVirtualWindows;
    p.ppb = k.ppb_user ? k.ppb_user : 7;
    if (!k.generic && !k.ppb_user)   // (N = 4096: blocks sized to this batch's work items)
        (void)split_cost4096(k.n_cus, k.n_buoys, a.n_pairs, (p.one_launch ? W * D : W) * M / a.integ, 0, &p.ppb);
    // The chunk of the per-hypothesis sweep.  Banded: on the generic routes plan_bands' chunk for M bands -- the cap of the
    // per-slot buffers, as plan_route takes it --; at N = 4096 chunk_windows, cut so that a chunk's virtual windows stay
    // below the pair grid's bound.  A window whose own M * P slots no chunk holds (the four-step column pass has one grid
    // row per slot, and its products lie under the budget) is refused, never split.
    const bool four_step = k.generic && (1L << k.logL) > k.small_maxl;
    long chunk = k.generic ? k.g_chunk : k.chunk_windows;
    if (M > 1) {
        if (k.generic) {
            chunk = plan_bands(k.g_chunk, W, (int)M, k.n_buoys, a.n_pairs, 1L << k.logL, four_step, 0, 0, 0).chunk;
            const long per_win = ((long)k.n_buoys + M * a.n_pairs) * (1L << k.logL) * 8;
            if (four_step && (M * a.n_pairs > kMaxGridY || per_win > kGenericBudgetBytes)) p.refused = kRefuseBandsChunk;
        } else if (chunk * M >= kCafMaxVirtualWindows) {
            chunk = (kCafMaxVirtualWindows - 1) / M;
        }
    } else if (four_step) {
        chunk = cap_chunk_grid_rows(chunk, 1, a.n_pairs, a.integ);   // as plan_route: g_cols_inv's grid rows, whole groups
    }
    if (p.refused == kRouteOk) p.refused = integ_chunk(k, (int)chunk, a.integ, four_step, &p.chunk);
    p.out_elems = (size_t)(W / a.integ) * (size_t)M * a.n_pairs;
    p.hyp_elems = p.one_launch ? p.out_elems * (size_t)D : p.out_elems;
    p.need_nb = a.fine && (!p.one_launch || !a.out_dev);
    p.stage_dfrac = a.fine && !a.out_dev;
    p.second_sweep = (a.refined || a.qualified) && !p.one_launch;
    return p;
}

}  // namespace host
}  // namespace rmx
