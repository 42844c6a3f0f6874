// Host-side logic of the C ABI (radio-mapper_amd/csrc/host_plan.hpp) under AddressSanitizer + UBSan.
// Built and run by tests/test_host_plan_sanitized.py:  g++ -std=c++17 -O1 -g -fsanitize=address,undefined
// -fno-sanitize-recover=all -o ... tests/host/test_host_plan.cpp ; exit code 0 = every check passed and neither
// sanitizer reported anything.
#include <cassert>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <thread>

#include "../../radio-mapper_amd/csrc/host_plan.hpp"

using namespace rmx;
using namespace rmx::host;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

static void test_options() {
    std::string why;
    clear_default_options();
    CHECK(set_default_option("wscr", 2, &why) == 0);
    CHECK(set_default_option("wscr", 3, &why) == -1 && why.find("not in 0..2") != std::string::npos);
    CHECK(set_default_option("no_such_key", 1, &why) == -1 && why.find("unknown option") != std::string::npos);
    CHECK(set_default_option(nullptr, 1, &why) == -1);
    CHECK(set_default_option("stag", 5, &why) == 0 && set_default_option("stag", 6, &why) == -1);
    Knobs snap = snapshot_default_options();
    long v = -1;
    CHECK(snap.get("wscr", &v) && v == 2 && snap.get_or("stag", 1) == 5 && snap.get_or("fused", 7) == 7);
    CHECK(set_default_option("wscr", LONG_MIN, &why) == 0);                 // removes the key ...
    CHECK(!snapshot_default_options().get("wscr", &v) && snap.get("wscr", &v));   // ... but not from an earlier snapshot
    // concurrent setters and snapshots (the store is shared by every thread that creates engines)
    std::vector<std::thread> th;
    for (int t = 0; t < 8; ++t)
        th.emplace_back([t] {
            std::string w;
            for (int i = 0; i < 2000; ++i) {
                set_default_option(t & 1 ? "fused" : "wfused", i & 1, &w);
                Knobs k = snapshot_default_options();
                (void)k.get_or("fused", 0);
            }
        });
    for (auto& x : th) x.join();
    clear_default_options();
    CHECK(snapshot_default_options().v.empty());
    for (const OptionSpec& s : option_specs()) CHECK(s.lo <= s.hi && s.key && s.what);
}

static void test_create_args() {
    std::string why;
    CHECK(check_create_args(8, 4096, 1, &why) == 0);
    CHECK(check_create_args(1, 4096, 1, &why) == -1 && why.find("n_buoys") != std::string::npos);
    CHECK(check_create_args(4097, 4096, 1, &why) == -1);
    CHECK(check_create_args(8, 4095, 1, &why) == -1 && check_create_args(8, 8, 1, &why) == -1);
    CHECK(check_create_args(8, 1 << 22, 1, &why) == 0 && check_create_args(8, 1 << 23, 1, &why) == -1);
    CHECK(check_create_args(8, 4096, 0, &why) == -1 && check_create_args(8, INT_MIN, 1, &why) == -1);
    CHECK(is_pow2(1) && is_pow2(1L << 40) && !is_pow2(0) && !is_pow2(-8) && !is_pow2(12));
}

static void test_pair_plan() {
    std::string why;
    for (int B = 2; B <= 33; ++B) {                                          // default plan of every buoy count
        for (int ppb : {1, 7, 0, 1000}) {
            PairPlan p;
            const int P = B * (B - 1) / 2;
            CHECK(make_pair_plan(B, nullptr, P, ppb, &p, &why) == 0);
            CHECK(p.all_pairs && (int)p.items.size() == P && (int)p.pairs.size() == 2 * P);
            CHECK(p.part_begin.front() == 0 && p.part_begin.back() == P && (int)p.part_begin.size() == p.n_parts + 1);
            const int eff = ppb > 0 ? ppb : 7;
            for (int k = 0; k < p.n_parts; ++k) CHECK(p.part_begin[k + 1] > p.part_begin[k] && p.part_begin[k + 1] - p.part_begin[k] <= eff);
            int q = 0;
            for (int i = 0; i < B; ++i)
                for (int j = i + 1; j < B; ++j, ++q) {
                    CHECK(p.items[q].i == i && p.items[q].j == j && p.items[q].out == q);
                    CHECK(p.items[q].run == B - j);                              // pairs left in anchor i's run
                }
        }
    }
    PairPlan p;
    CHECK(make_pair_plan(8, nullptr, 27, 7, &p, &why) == -1 && why.find("pairs == NULL") != std::string::npos);
    CHECK(make_pair_plan(8, nullptr, -1, 7, &p, &why) == -1);
    const int32_t bad1[] = {0, 1, 2, 8}, bad2[] = {-1, 0}, ok0[] = {7, 0, 0, 1, 1, 1, 0, 1};
    CHECK(make_pair_plan(8, bad1, 2, 7, &p, &why) == -1 && why.find("pair 1 = (2,8)") != std::string::npos);
    CHECK(make_pair_plan(8, bad2, 1, 7, &p, &why) == -1);
    CHECK(make_pair_plan(8, ok0, 4, 7, &p, &why) == 0 && !p.all_pairs && p.n_parts == 1);   // reversed, repeated, autocorrelation
    CHECK(p.items[0].run == 1 && p.items[1].run == 1 && p.items[2].run == 1 && p.items[3].run == 1);
    CHECK(make_pair_plan(8, ok0, 0, 7, &p, &why) == 0 && p.n_parts == 0 && p.items.empty() && p.part_begin.size() == 1);
    // the default list passed explicitly is recognised as the default plan; one swap is not
    std::vector<int32_t> pl;
    for (int i = 0; i < 5; ++i) for (int j = i + 1; j < 5; ++j) { pl.push_back(i); pl.push_back(j); }
    CHECK(make_pair_plan(5, pl.data(), 10, 7, &p, &why) == 0 && p.all_pairs);
    std::swap(pl[2], pl[3]);
    CHECK(make_pair_plan(5, pl.data(), 10, 7, &p, &why) == 0 && !p.all_pairs);
    // random lists: runs are consistent, parts cover everything once
    std::mt19937 rng(7);
    for (int trial = 0; trial < 200; ++trial) {
        const int B = 2 + rng() % 30, P = rng() % 200, ppb = 1 + rng() % 12;
        std::vector<int32_t> r(2 * (size_t)P + 2);                             // (+2: a non-NULL pointer also for P = 0)
        for (auto& x : r) x = (int32_t)(rng() % B);
        CHECK(make_pair_plan(B, r.data(), P, ppb, &p, &why) == 0);
        for (int q = 0; q + 1 < P; ++q)
            CHECK(p.items[q].run == (p.items[q].i == p.items[q + 1].i ? p.items[q + 1].run + 1 : 1));
        if (P) CHECK(p.items[P - 1].run == 1 && p.part_begin.back() == P);
    }
}

static void test_chunks() {
    // cfg2: 3 buoys, L = 2^21, 64 windows -> one chunk; the cap and the 4096 limit; never below one window
    {   // the N = 4096 dispatch model: the measured crossovers of tools/exp_small4096.py, and no way to break it
        int q = 0;
        CHECK(split_cost4096(256, 8, 28, 1, 0, &q) < fused_cost4096(256, 8, 28, 1) && q == 1);        // one group: per-transform, 1 pair per block
        CHECK(split_cost4096(256, 16, 120, 1, 0, &q) < fused_cost4096(256, 16, 120, 1) && q == 1);
        CHECK(split_cost4096(256, 8, 28, 64, 0, &q) < fused_cost4096(256, 8, 28, 64) && q == 7);      // 64 windows: 7 pairs per block
        CHECK(split_cost4096(256, 8, 28, 256, 0, &q) > fused_cost4096(256, 8, 28, 256));              // a full round: fused
        CHECK(split_cost4096(256, 3, 3, 128, 0, &q) > fused_cost4096(256, 3, 3, 128));
        CHECK(split_cost4096(256, 3, 3, 32, 0, &q) < fused_cost4096(256, 3, 3, 32));
        CHECK(split_cost4096(256, 8, 28, 4, 5, &q) > 0 && q == 5);                                    // the caller's block size is kept
        for (int cus : {0, 1, 7, 256, 4096})
            for (long w : {0L, 1L, 255L, 256L, 257L, 1L << 20})
                for (int b : {2, 3, 64})
                    for (int fixed : {0, 1, 1 << 20}) {
                        const int pairs = b * (b - 1) / 2;
                        const double t = split_cost4096(cus, b, pairs, w, fixed, &q), f = fused_cost4096(cus, b, pairs, w);
                        CHECK(t > 0 && t < 1e30 && f > 0 && q >= 1 && (fixed ? q == fixed : q <= 7));
                    }
        CHECK(split_cost4096(256, 4, 0, 3, 0, &q) > 0 && q >= 1);                                     // an empty pair list divides by nothing
    }
    CHECK(generic_chunk_windows(3, 1L << 21, 64, 32L << 30, 0) == 64);
    CHECK(generic_chunk_windows(3, 1L << 21, 64, 32L << 30, 16) == 16);
    CHECK(generic_chunk_windows(32, 1L << 19, 64, 32L << 30, 0) == (32L << 30) / ((32 + 496) * (1L << 19) * 8));
    CHECK(generic_chunk_windows(8, 512, 1 << 20, 32L << 30, 0) == 4096);
    CHECK(generic_chunk_windows(4096, 1L << 23, 5, 1 << 20, 0) == 1);
    CHECK(generic_chunk_windows(2, 32, 1, 32L << 30, 4096) == 1);
}

static void test_request_conversions() {
    int32_t a = 77, b = 77;
    for (int N : {16, 4096, 1 << 22}) {
        const double L = 2.0 * N;
        CHECK(band_to_bins(-0.5, 0.5, N, &a, &b) == kBandOk && a == -N && b == N - 1);            // the full band
        CHECK(band_to_bins(0.25, 0.5, N, &a, &b) == kBandOk && a == N / 2 && b == N - 1);         // hi = 0.5 is bin N: clamped
        CHECK(band_to_bins(0.5, 0.5, N, &a, &b) == kBandNoBin);                                   // ... and on its own keeps nothing
        CHECK(band_to_bins(-0.5, -0.5, N, &a, &b) == kBandOk && a == -N && b == -N);
        CHECK(band_to_bins(0.0, 0.0, N, &a, &b) == kBandOk && a == 0 && b == 0);                  // one bin, both ends included
        CHECK(band_to_bins(3.0 / L, 5.0 / L, N, &a, &b) == kBandOk && a == 3 && b == 5);
        CHECK(band_to_bins(-4.75 / L, 4.75 / L, N, &a, &b) == kBandOk && a == -4 && b == 4);      // inwards on both sides
        a = b = 77;
        CHECK(band_to_bins(1.25 / L, 1.75 / L, N, &a, &b) == kBandNoBin && a == 77 && b == 77);   // between two adjacent bins
        CHECK(band_to_bins(-1.75 / L, -1.25 / L, N, &a, &b) == kBandNoBin);
        CHECK(band_to_bins(0.1, 0.05, N, &a, &b) == kBandNoInterval);                             // lo > hi
        CHECK(band_to_bins(-0.5000001, 0.0, N, &a, &b) == kBandNoInterval && band_to_bins(0.0, 0.5000001, N, &a, &b) == kBandNoInterval);
        CHECK(band_to_bins(NAN, 0.1, N, &a, &b) == kBandNoInterval && band_to_bins(0.0, INFINITY, N, &a, &b) == kBandNoInterval);
        CHECK(band_to_bins(-INFINITY, 0.0, N, &a, &b) == kBandNoInterval && a == 77 && b == 77);
    }
    bool full = false;
    for (int N : {16, 4096, 1 << 22}) {
        const int nm1 = N - 1;
        CHECK(lag_interval_ok(-nm1, nm1, N, &full) && full);
        CHECK(lag_interval_ok(-nm1 + 1, nm1, N, &full) && !full && lag_interval_ok(-nm1, nm1 - 1, N, &full) && !full);
        CHECK(lag_interval_ok(5, 5, N, &full) && !full && lag_interval_ok(-nm1, -nm1, N, &full) && lag_interval_ok(nm1, nm1, N, &full));
        CHECK(!lag_interval_ok(-nm1 - 1, 0, N, &full) && !lag_interval_ok(-N, nm1, N, &full));   // lo < -(N-1)
        CHECK(!lag_interval_ok(0, N, N, &full) && !lag_interval_ok(3, 2, N, &full));
        CHECK(!lag_interval_ok(INT_MIN, INT_MAX, N, &full) && !lag_interval_ok(INT_MAX, INT_MIN, N, &full));
    }
}

// ---- the route planner -------------------------------------------------------------------------------------------------
// the caps rmx_create gives an N = 4096 ctx: every one follows from (buoys, max_windows, ncus, options) without a device
static RouteCaps caps4096(int n_buoys, int max_windows, int n_cus, int chunk_opt = 4096) {
    RouteCaps k;
    k.n_cus = n_cus;
    k.n_buoys = n_buoys;
    int chunk = chunk_opt < 8 ? 8 : chunk_opt;
    chunk = (chunk + 7) & ~7;
    if (chunk > max_windows) chunk = max_windows;
    k.chunk_windows = chunk;
    return k;
}
static RouteCall call4096(int n_buoys, int n_windows) {
    RouteCall a;
    a.n_windows = n_windows;
    a.n_pairs = n_buoys * (n_buoys - 1) / 2;
    a.in_dev = false;
    return a;
}
// the launches of families "k_fwd" and "k_win|k_pair" a plan implies for a plain N = 4096 call
static void launches4096(const RouteCaps& k, const RouteCall& a, int* n_fwd, int* n_pair, RoutePlan* out = nullptr) {
    const RoutePlan p = plan_route(k, a);
    CHECK(p.refused == kRouteOk && p.chunk > 0);
    *n_fwd = *n_pair = 0;
    for (int w0 = 0; w0 < a.n_windows; w0 += p.chunk) {
        const int wc = a.n_windows - w0 < p.chunk ? a.n_windows - w0 : p.chunk;
        if (p.route == kRoutePer4096) { ++*n_fwd; ++*n_pair; continue; }
        CHECK(p.route == kRouteKWin);
        const int wtail = route_wtail4096(k, p, a.n_pairs, w0, wc), wf = wc - wtail;
        if (wf > 0) *n_pair += p.pipelined ? (wf + kHostSubChunk - 1) / kHostSubChunk : 1;
        if (wtail) { ++*n_fwd; ++*n_pair; }
    }
    if (out) *out = p;
}

// The N = 4096 rows of tests/golden/route_table.json, transcribed: the launch counts are the RECORDING's (the library of the
// commit before the planner, on an MI355X), the plan must imply exactly them.  pairs: 0 the default list (NULL), 1 the default
// list passed explicitly, 2 the default list reversed, 3 the default list without its last pair.  quality_only: the two-pass
// route (the plain call, then one k_fwd per chunk in front of k_quality).
struct RecordedRow {
    const char* name;
    int B, W, max_windows, ncus, chunk_opt;
    bool fused, small4096;
    int ppb_user, pairs;
    bool bounded, weighted;
    int integ;
    bool in_dev, quality_only;
    int k_fwd, k_pair;   // launches of the families "k_fwd" and "k_win|k_pair"
};
static const RecordedRow kRecorded[] = {
    {"n4096_b3_w1", 3, 1, 1, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 1, 1},
    {"n4096_b3_w2", 3, 2, 2, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 1, 1},
    {"n4096_b3_w4", 3, 4, 4, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b3_w8", 3, 8, 8, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b3_w12", 3, 12, 12, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b3_w9_tail", 3, 9, 9, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 1, 2},
    {"n4096_b3_w15_tail", 3, 15, 15, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b3_w17_tail", 3, 17, 17, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 1, 2},
    {"n4096_b3_w23_tail", 3, 23, 23, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b3_w15_chunk8_cu6", 3, 15, 15, 6, 8, true, true, 0, 0, false, false, 1, false, false, 1, 3},
    {"n4096_b3_w14_chunk8_cu6", 3, 14, 14, 6, 8, true, true, 0, 0, false, false, 1, false, false, 0, 2},
    {"n4096_b3_w17_rev", 3, 17, 17, 8, 4096, true, true, 0, 2, false, false, 1, false, false, 1, 1},
    {"n4096_b3_w17_explicit_default", 3, 17, 17, 8, 4096, true, true, 0, 1, false, false, 1, false, false, 1, 2},
    {"n4096_b3_w4_sub", 3, 4, 4, 8, 4096, true, true, 0, 3, false, false, 1, false, false, 1, 1},
    {"n4096_b3_w17_unfused", 3, 17, 17, 8, 4096, false, true, 0, 0, false, false, 1, false, false, 1, 1},
    {"n4096_b3_w17_ppb3", 3, 17, 17, 8, 4096, true, true, 3, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b3_w2_ppb3", 3, 2, 2, 8, 4096, true, true, 3, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b3_w17_small0", 3, 17, 17, 8, 4096, true, false, 0, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b3_w2_small0", 3, 2, 2, 8, 4096, true, false, 0, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b3_w17_u8", 3, 17, 17, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 1, 2},
    {"n4096_b3_w17_bounded", 3, 17, 17, 8, 4096, true, true, 0, 0, true, false, 1, false, false, 1, 2},
    {"n4096_b8_w1", 8, 1, 1, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 1, 1},
    {"n4096_b8_w2", 8, 2, 2, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 1, 1},
    {"n4096_b8_w4", 8, 4, 4, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 1, 1},
    {"n4096_b8_w8", 8, 8, 8, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b8_w12", 8, 12, 12, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 1, 2},
    {"n4096_b8_w9_tail", 8, 9, 9, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 1, 2},
    {"n4096_b8_w15_tail", 8, 15, 15, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b8_w17_tail", 8, 17, 17, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 1, 2},
    {"n4096_b8_w23_tail", 8, 23, 23, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b8_w15_chunk8_cu6", 8, 15, 15, 6, 8, true, true, 0, 0, false, false, 1, false, false, 2, 4},
    {"n4096_b8_w14_chunk8_cu6", 8, 14, 14, 6, 8, true, true, 0, 0, false, false, 1, false, false, 1, 3},
    {"n4096_b8_w17_rev", 8, 17, 17, 8, 4096, true, true, 0, 2, false, false, 1, false, false, 1, 1},
    {"n4096_b8_w17_explicit_default", 8, 17, 17, 8, 4096, true, true, 0, 1, false, false, 1, false, false, 1, 2},
    {"n4096_b8_w4_sub", 8, 4, 4, 8, 4096, true, true, 0, 3, false, false, 1, false, false, 1, 1},
    {"n4096_b8_w17_unfused", 8, 17, 17, 8, 4096, false, true, 0, 0, false, false, 1, false, false, 1, 1},
    {"n4096_b8_w17_ppb3", 8, 17, 17, 8, 4096, true, true, 3, 0, false, false, 1, false, false, 1, 2},
    {"n4096_b8_w2_ppb3", 8, 2, 2, 8, 4096, true, true, 3, 0, false, false, 1, false, false, 1, 1},
    {"n4096_b8_w17_small0", 8, 17, 17, 8, 4096, true, false, 0, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b8_w2_small0", 8, 2, 2, 8, 4096, true, false, 0, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b8_w17_u8", 8, 17, 17, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 1, 2},
    {"n4096_b8_w17_bounded", 8, 17, 17, 8, 4096, true, true, 0, 0, true, false, 1, false, false, 1, 2},
    {"n4096_b2_w3", 2, 3, 3, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 0, 1},
    {"n4096_b3_w521_host", 3, 521, 521, 8, 4096, true, true, 0, 0, false, false, 1, false, false, 0, 2},
    {"n4096_b3_w521_device", 3, 521, 521, 8, 4096, true, true, 0, 0, false, false, 1, true, false, 1, 2},
    {"n4096_bounded", 3, 6, 6, 8, 4096, true, true, 0, 0, true, false, 1, false, false, 0, 1},
    {"n4096_band_phat", 3, 6, 6, 8, 4096, true, true, 0, 0, false, true, 1, false, false, 1, 1},
    {"n4096_integ2", 3, 6, 6, 8, 4096, true, true, 0, 0, true, true, 2, false, false, 1, 1},
    {"n4096_refine4", 3, 6, 6, 8, 4096, true, true, 0, 0, false, true, 1, false, false, 1, 1},
    {"n4096_quality", 3, 6, 6, 8, 4096, true, true, 0, 0, false, false, 1, false, true, 1, 1},
    {"n4096_quality_band", 3, 6, 6, 8, 4096, true, true, 0, 0, false, true, 1, false, false, 1, 1},
    {"n4096_all", 3, 6, 6, 8, 4096, true, true, 0, 0, true, true, 2, false, false, 1, 1},
    {"n4096_all_two_chunks", 3, 16, 16, 8, 8, true, true, 0, 0, true, true, 2, false, false, 2, 2},
    {"n4096_quality_two_chunks", 3, 16, 16, 8, 8, true, true, 0, 0, false, false, 1, false, true, 2, 2},
    {"n4096_plain_two_chunks", 3, 16, 16, 8, 8, true, true, 0, 0, false, false, 1, false, false, 0, 2},
};

static void test_recorded_rows() {
    int n = 0;
    for (const RecordedRow& r : kRecorded) {
        RouteCaps k = caps4096(r.B, r.max_windows, r.ncus, r.chunk_opt);
        k.fused = r.fused;
        k.small_batch = r.small4096;
        k.ppb_user = r.ppb_user;
        RouteCall a = call4096(r.B, r.W);
        if (r.pairs == 3) --a.n_pairs;
        a.all_pairs = r.pairs < 2;
        a.pairs_given = r.pairs != 0;
        a.bounded = r.bounded;
        a.weighted = r.weighted;
        a.integ = r.integ;
        a.in_dev = r.in_dev;
        int n_fwd = 0, n_pair = 0;
        RoutePlan p;
        launches4096(k, a, &n_fwd, &n_pair, &p);
        if (r.quality_only) n_fwd += (r.W + k.chunk_windows - 1) / k.chunk_windows;
        if (n_fwd != r.k_fwd || n_pair != r.k_pair) {
            std::fprintf(stderr, "%s: the plan implies %d k_fwd + %d k_win|k_pair launches, recorded %d + %d\n", r.name, n_fwd, n_pair,
                         r.k_fwd, r.k_pair);
            std::exit(1);
        }
        if (r.ppb_user) CHECK(p.ppb == r.ppb_user);
        ++n;
    }
    CHECK(n >= 40);
}


static bool same_plan(const RoutePlan& a, const RoutePlan& b) {
    return a.route == b.route && a.ppb == b.ppb && a.chunk == b.chunk && a.n_head == b.n_head && a.n_tail == b.n_tail && a.tail == b.tail &&
           a.pipelined == b.pipelined && a.refused == b.refused;
}

static void test_route_invariants() {
    long n_plans = 0;
    for (int B = 2; B <= 16; ++B)
        for (int logL = 5; logL <= 23; ++logL)
            for (int n_cus : {1, 8, 37})
                for (int variant = 0; variant < 4; ++variant) {
                    RouteCaps k;
                    k.n_cus = n_cus;
                    k.n_buoys = B;
                    k.generic = !(logL == 13 && variant < 2);                     // (logL 13: N = 4096 itself, and generic4096)
                    k.logL = logL;
                    k.small_maxl = 8192;
                    k.fused = variant != 1;
                    k.chunk_windows = variant == 0 ? 4096 : 8;
                    k.ppb_user = variant == 1 ? 9 : 0;
                    if (k.generic) {                                                // as generic_init derives them
                        const bool four_step = (1L << logL) > k.small_maxl;
                        if (four_step) {
                            k.logL1 = (logL - 3) / 2;
                            if (k.logL1 < logL - 13) k.logL1 = logL - 13;
                            if (k.logL1 > 10) k.logL1 = 10;
                            k.logL2 = logL - k.logL1;
                            k.g_fused = B <= 4 && k.logL2 >= 9 && k.logL2 <= 12 && variant != 3;
                            k.g_fused_always = k.g_fused && variant == 2;
                            k.col_tile = (1L << k.logL1) << (k.logL1 >= 10 ? 3 : 4);
                            k.cols_threads = variant == 3 ? 64 : (int)(k.col_tile / 16 >= 1024 ? 1024 : k.col_tile / 16 < 64 ? 64 : k.col_tile / 16);
                        }
                        k.wfused = !four_step && B <= 4 && logL >= 9 && logL <= 12 && variant != 3;
                        k.wscr = !k.wfused && logL >= 9 && logL <= 15 && variant != 3;
                        k.wscr_always = k.wscr && variant == 2;
                        k.ws_upw = logL >= 13 ? 1 : 2;
                        k.ws_grid = n_cus;
                        k.k8 = k.wscr && logL == 14 && variant != 1;
                        k.k16 = k.wscr && logL == 15 ? (variant == 1 ? 2 : 1) : 0;
                        k.g_chunk = variant == 3 ? 3 : 64;
                    }
                    const int P = B * (B - 1) / 2;
                    for (int W = 1; W <= 3 * n_cus + 1; ++W)
                        for (int flags = 0; flags < 8; ++flags)
                            for (int integ : {1, 2, 5}) {
                                RouteCall a;
                                a.n_windows = W;
                                a.all_pairs = !(flags & 4);
                                a.pairs_given = flags & 4;
                                const int custom[3] = {640, 641, 700};               // at, just beyond and far beyond kMaxPairs8 / kMaxPairs16
                                a.n_pairs = a.all_pairs ? P : custom[(W + integ) % 3];
                                a.bounded = (flags & 1) || integ > 1;               // (an integrated call always carries bounds)
                                a.weighted = (flags & 2) || integ > 1;
                                a.integ = integ;
                                a.in_dev = W & 1;
                                if (W % integ != 0) continue;                       // (refused by the entry)
                                const RoutePlan p = plan_route(k, a);
                                ++n_plans;
                                if (a.n_pairs > 640) CHECK(p.route != kRouteKWin8 && p.route != kRouteK16);
                                CHECK(same_plan(p, plan_route(k, a)));              // a pure function
                                const bool whole = p.route == kRouteKWin || p.route == kRouteKWin8 || p.route == kRouteWinScr ||
                                                   p.route == kRouteWinEo15 || p.route == kRouteWinFused;
                                CHECK(k.generic == !(p.route == kRouteKWin || p.route == kRoutePer4096));
                                if (a.weighted) {
                                    CHECK(!whole && p.route != kRouteK16);
                                    for (int wc = 1; wc <= W; ++wc) CHECK(!route_rows_fused(k, true, wc));
                                }
                                // only k_win, k_win8kl, k16_pairs and the per-transform kernels have a bounded instantiation
                                if (a.bounded) CHECK(p.route != kRouteWinScr && p.route != kRouteWinEo15 && p.route != kRouteWinFused);
                                if (k.generic) {
                                    CHECK(p.n_head + p.n_tail == W && p.n_tail >= 0);
                                    if (p.n_tail) CHECK(p.n_head > 0 && p.n_head % k.ws_grid == 0 && (p.route == kRouteKWin8 || p.route == kRouteWinEo15));
                                }
                                const bool chunked = p.route == kRoutePer4096 || p.route == kRouteKWin || p.route == kRouteSmallL ||
                                                     p.route == kRouteFourStep;
                                if (chunked) CHECK(p.refused != kRouteOk || (p.chunk > 0 && p.chunk % integ == 0));
                                if (p.refused != kRouteOk) CHECK(integ > 1 && !whole);
                                if (p.refused == kRefuseIntegChunk) CHECK(integ > (k.generic ? k.g_chunk : k.chunk_windows));
                                if (!k.generic) CHECK(k.ppb_user ? p.ppb == k.ppb_user : (p.ppb >= 1 && p.ppb <= 7));
                                if (p.route != kRouteKWin) CHECK(p.tail == 0 && !p.pipelined);
                                if (p.route == kRouteKWin && p.refused == kRouteOk)
                                    for (int w0 = 0; w0 < W; w0 += p.chunk) {
                                        const int wc = W - w0 < p.chunk ? W - w0 : p.chunk;
                                        const int wtail = route_wtail4096(k, p, a.n_pairs, w0, wc);
                                        CHECK(0 <= wtail && wtail < k.n_cus && wtail <= wc);
                                        if (!p.tail) CHECK(wtail == 0);
                                    }
                            }
                }
    CHECK(n_plans > 100000);
    // the pipelined host copy: only k_win, only host windows beyond one sub-chunk; the tail gate is then closed
    RouteCaps k = caps4096(3, 4096, 8);
    RouteCall a = call4096(3, kHostSubChunk + 9);
    CHECK(plan_route(k, a).pipelined && plan_route(k, a).tail == 0);
    a.in_dev = true;
    CHECK(!plan_route(k, a).pipelined && plan_route(k, a).tail == 1);
    a.n_windows = kHostSubChunk;
    a.in_dev = false;
    CHECK(!plan_route(k, a).pipelined);
    // a custom list of exactly kMaxPairs8 / kMaxPairs16 pairs still takes k_win8kl / k16, one more does not
    for (int logL : {14, 15}) {
        RouteCaps g;
        g.generic = true;  g.n_cus = 8;  g.n_buoys = 8;  g.logL = logL;  g.logL1 = logL - 10;  g.logL2 = 10;  g.g_chunk = 64;
        g.wscr = true;  g.ws_upw = 1;  g.ws_grid = 8;  g.k8 = logL == 14;  g.k16 = logL == 15;
        RouteCall b;
        b.n_windows = 8;  b.all_pairs = false;  b.pairs_given = true;
        b.n_pairs = 640;
        CHECK(plan_route(g, b).route == (logL == 14 ? kRouteKWin8 : kRouteK16));
        b.n_pairs = 641;
        CHECK(plan_route(g, b).route == (logL == 14 ? kRouteWinScr : kRouteWinEo15));
    }
    // the default list is recognised with and without a pointer, and nothing is read when the count is off
    const int32_t d3[] = {0, 1, 0, 2, 1, 2}, s3[] = {0, 2, 0, 1, 1, 2};
    CHECK(is_default_list(3, nullptr, 3) && is_default_list(3, d3, 3) && !is_default_list(3, s3, 3) && !is_default_list(3, nullptr, 2) &&
          !is_default_list(3, d3, 2));
}

// ---- the Doppler search: plan_caf ----------------------------------------------------------------------------------------
// The rows of tests/golden/caf_route_table.json, transcribed (three hypotheses unless D says otherwise; ncus = 8): the launch
// counts are the RECORDING's (the library of the commit before plan_caf, on an MI355X), the plan must imply exactly them.
// chunk: chunk_windows as rmx_create derives it (caps4096), or g_chunk of a generic ctx (gen_chunk, else max_windows = W).
// fwd: launches of each forward family (k_fwd; g_fwd_small; g_cols_fwd and g_rows_fwd each); pair: of each pair family
// (k_win|k_pair; g_pair_small; g_cols_inv, g_rows_inv and g_final each); then k_caf_select, k_quality, k_refine.
struct RecordedCaf {
    const char* name;
    int B, W, D, K, logL;       // logL = 0: N = 4096 on its own kernels
    int chunk_opt, ppb_user;
    bool fine, refined, qualified, out_dev;
    int fwd, pair, select, quality, refine;
    RouteRefusal refused;
};
static const RecordedCaf kRecordedCaf[] = {
    {"caf_n256_fine", 3, 4, 3, 1, 9, 0, 0, true, false, false, false, 4, 3, 3, 0, 0, kRouteOk},
    {"caf_n256_bounded_band_phat", 3, 4, 3, 1, 9, 0, 0, false, false, false, false, 4, 3, 3, 0, 0, kRouteOk},
    {"caf_n256_integ2", 3, 4, 3, 2, 9, 0, 0, false, false, false, false, 4, 3, 3, 0, 0, kRouteOk},
    {"caf_n256_refine4_quality", 3, 4, 3, 1, 9, 0, 0, false, true, true, false, 7, 3, 3, 3, 3, kRouteOk},
    {"caf_n256_all", 3, 4, 3, 2, 9, 0, 0, true, true, true, false, 7, 3, 3, 3, 3, kRouteOk},
    {"caf_n256_all_two_chunks", 3, 8, 3, 2, 9, 4, 0, true, true, true, false, 14, 6, 6, 6, 6, kRouteOk},
    {"caf_n4096_one_fine", 3, 4, 3, 1, 0, 4096, 0, true, false, false, false, 2, 1, 1, 0, 0, kRouteOk},
    {"caf_n4096_one_bounded_band_phat", 3, 4, 3, 1, 0, 4096, 0, false, false, false, false, 2, 1, 1, 0, 0, kRouteOk},
    {"caf_n4096_one_integ2", 3, 4, 3, 2, 0, 4096, 0, false, false, false, false, 2, 1, 1, 0, 0, kRouteOk},
    {"caf_n4096_one_refine4_quality", 3, 4, 3, 1, 0, 4096, 0, false, true, true, false, 2, 1, 1, 1, 1, kRouteOk},
    {"caf_n4096_one_all", 3, 4, 3, 2, 0, 4096, 0, true, true, true, false, 2, 1, 1, 1, 1, kRouteOk},
    {"caf_n4096_per_fine", 3, 12, 3, 1, 0, 8, 0, true, false, false, false, 8, 6, 6, 0, 0, kRouteOk},
    {"caf_n4096_per_bounded_band_phat", 3, 12, 3, 1, 0, 8, 0, false, false, false, false, 8, 6, 6, 0, 0, kRouteOk},
    {"caf_n4096_per_integ2", 3, 12, 3, 2, 0, 8, 0, false, false, false, false, 8, 6, 6, 0, 0, kRouteOk},
    {"caf_n4096_per_refine4_quality", 3, 12, 3, 1, 0, 8, 0, false, true, true, false, 14, 6, 6, 6, 6, kRouteOk},
    {"caf_n4096_per_all", 3, 12, 3, 2, 0, 8, 0, true, true, true, false, 14, 6, 6, 6, 6, kRouteOk},
    {"caf_n4096_per_all_two_chunks", 3, 16, 3, 2, 0, 8, 0, true, true, true, false, 14, 6, 6, 6, 6, kRouteOk},
    {"caf_n8192_fine", 3, 4, 3, 1, 14, 0, 0, true, false, false, false, 4, 3, 3, 0, 0, kRouteOk},
    {"caf_n8192_bounded_band_phat", 3, 4, 3, 1, 14, 0, 0, false, false, false, false, 4, 3, 3, 0, 0, kRouteOk},
    {"caf_n8192_integ2", 3, 4, 3, 2, 14, 0, 0, false, false, false, false, 4, 3, 3, 0, 0, kRouteOk},
    {"caf_n8192_refine4_quality", 3, 4, 3, 1, 14, 0, 0, false, true, true, false, 7, 3, 3, 3, 3, kRouteOk},
    {"caf_n8192_all", 3, 4, 3, 2, 14, 0, 0, true, true, true, false, 7, 3, 3, 3, 3, kRouteOk},
    {"caf_n8192_all_two_chunks", 3, 8, 3, 2, 14, 4, 0, true, true, true, false, 14, 6, 6, 6, 6, kRouteOk},
    {"caf_n4096_single", 3, 4, 1, 1, 0, 4096, 0, false, false, false, false, 2, 1, 1, 0, 0, kRouteOk},
    {"caf_n4096_one_fine_device", 3, 4, 3, 1, 0, 4096, 0, true, false, false, true, 2, 1, 1, 0, 0, kRouteOk},
    {"caf_n4096_per_fine_device", 3, 12, 3, 1, 0, 8, 0, true, false, false, true, 8, 6, 6, 0, 0, kRouteOk},
    {"caf_n4096_u8", 3, 4, 3, 1, 0, 4096, 0, false, false, false, false, 2, 1, 1, 0, 0, kRouteOk},
    {"caf_n4096_generic", 3, 4, 3, 1, 13, 0, 0, false, false, false, false, 4, 3, 3, 0, 0, kRouteOk},
    {"caf_n4096_rev", 3, 4, 3, 1, 0, 4096, 0, false, false, false, false, 2, 1, 1, 0, 0, kRouteOk},
    {"caf_n4096_b8_ppb3_integ2", 8, 4, 3, 2, 0, 4096, 3, false, false, false, false, 2, 1, 1, 0, 0, kRouteOk},
    {"caf_n4096_integ16_chunk8", 3, 16, 3, 16, 0, 8, 0, false, false, false, false, 0, 0, 0, 0, 0, kRefuseIntegChunk},
    {"caf_n8192_integ2_chunk1", 3, 4, 3, 2, 14, 1, 0, false, false, false, false, 0, 0, 0, 0, 0, kRefuseIntegChunk},
    {"caf_n65536_integ2_cols64", 3, 4, 3, 2, 17, 0, 0, false, false, false, false, 0, 0, 0, 0, 0, kRefuseIntegTile},
};

static bool same_caf_plan(const CafPlan& a, const CafPlan& b) {
    return a.one_launch == b.one_launch && a.ppb == b.ppb && a.chunk == b.chunk && a.refused == b.refused && a.out_elems == b.out_elems &&
           a.hyp_elems == b.hyp_elems && a.need_nb == b.need_nb && a.stage_dfrac == b.stage_dfrac && a.second_sweep == b.second_sweep;
}

static void test_recorded_caf_rows() {
    int n = 0, n_one = 0;
    for (const RecordedCaf& r : kRecordedCaf) {
        RouteCaps k = caps4096(r.B, r.W, 8, r.chunk_opt);
        k.ppb_user = r.ppb_user;
        if (r.logL) {
            k.generic = true;
            k.logL = r.logL;
            k.g_chunk = r.chunk_opt ? r.chunk_opt : r.W;
            if (r.logL == 17) { k.col_tile = 2048; k.cols_threads = 64; }   // (the recorded text: 2048 elements on 64 threads)
        }
        const CafCall a{r.W, r.B * (r.B - 1) / 2, r.D, r.K, r.fine, r.refined, r.qualified, r.out_dev};
        const CafPlan p = plan_caf(k, a);
        CHECK(p.refused == r.refused);
        ++n;
        if (p.refused != kRouteOk) continue;
        int fwd = 2, pair = 1, select = 1, quality = r.qualified, refine = r.refined;
        if (!p.one_launch) {
            const int chunks = (r.W + p.chunk - 1) / p.chunk, tail = p.second_sweep ? chunks * r.D : 0;
            fwd = chunks * (1 + r.D) + tail;
            pair = select = chunks * r.D;
            quality = r.qualified ? tail : 0;
            refine = r.refined ? tail : 0;
        }
        if (fwd != r.fwd || pair != r.pair || select != r.select || quality != r.quality || refine != r.refine) {
            std::fprintf(stderr, "%s: the plan implies %d forward, %d pair, %d select, %d quality, %d refine launches, recorded %d %d %d %d %d\n",
                         r.name, fwd, pair, select, quality, refine, r.fwd, r.pair, r.select, r.quality, r.refine);
            std::exit(1);
        }
        if (r.ppb_user) CHECK(p.ppb == r.ppb_user);
        CHECK(p.need_nb == (r.fine && !(p.one_launch && r.out_dev)));   // the two sides of the caf_nb rule: the two _device rows
        n_one += p.one_launch;
    }
    CHECK(n == 33 && n_one == 9);
}

static void test_caf_thresholds() {
    // at most 1 GiB of de-rotated spectra: 3 buoys x 8 windows x 64 KiB x D
    RouteCaps k = caps4096(3, 8, 8);
    CafCall a;
    a.n_windows = 8;  a.n_pairs = 3;
    a.n_dopplers = 682;
    CHECK(plan_caf(k, a).one_launch && plan_caf(k, a).hyp_elems == (size_t)8 * 3 * 682);
    a.n_dopplers = 683;
    CHECK(!plan_caf(k, a).one_launch && plan_caf(k, a).hyp_elems == (size_t)8 * 3);
    // D > 1, and one chunk
    a.n_dopplers = 1;
    CHECK(!plan_caf(k, a).one_launch);
    a.n_dopplers = 2;
    CHECK(plan_caf(k, a).one_launch);
    k = caps4096(3, 16, 8, 8);
    a.n_windows = 9;
    CHECK(!plan_caf(k, a).one_launch);
    a.n_windows = 8;
    CHECK(plan_caf(k, a).one_launch);
    k.generic = true;
    CHECK(!plan_caf(k, a).one_launch);
    // D * W < 2^20 virtual windows: with two or more buoys the 1 GiB above is reached first (D * W * B <= 2^14), so from
    // either side of 2^20 the answer is the same -- the bound only guards the launch arithmetic should the other ever move
    k = caps4096(3, 1024, 8);
    a.n_windows = 1023;  a.n_dopplers = 1025;   // 2^20 - 1
    CHECK((long)a.n_windows * a.n_dopplers == (1L << 20) - 1 && !plan_caf(k, a).one_launch);
    a.n_windows = 1024;  a.n_dopplers = 1024;   // 2^20
    CHECK(!plan_caf(k, a).one_launch);
}

static void test_caf_invariants() {
    long n_plans = 0;
    for (int B : {2, 3, 8})
        for (int generic = 0; generic < 3; ++generic)                                  // N = 4096 / small L / four-step
            for (int chunk : {1, 3, 8, 64})
                for (int ppb_user : {0, 9})
                    for (int W = 1; W <= 20; ++W)
                        for (int D : {1, 2, 3, 21, 683, 4096})
                            for (int K : {1, 2, 5})
                                for (int flags = 0; flags < 16; ++flags) {
                                    if (W % K != 0) continue;                           // (refused by the entry)
                                    RouteCaps k;
                                    k.n_cus = 8;  k.n_buoys = B;  k.generic = generic != 0;  k.logL = generic == 2 ? 14 : 13;
                                    k.chunk_windows = k.g_chunk = chunk;  k.ppb_user = ppb_user;
                                    k.col_tile = 512;  k.cols_threads = flags & 1 ? 64 : 16;   // 16 threads: 32 per thread, refused
                                    const int P = B * (B - 1) / 2;
                                    const CafCall a{W, P, D, K, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0};
                                    const CafPlan p = plan_caf(k, a);
                                    ++n_plans;
                                    CHECK(same_caf_plan(p, plan_caf(k, a)));            // a pure function
                                    CHECK(p.refused != kRouteOk || (p.chunk > 0 && p.chunk % K == 0 && p.chunk <= chunk));
                                    if (p.refused != kRouteOk) CHECK(K > 1);
                                    CHECK((p.refused == kRefuseIntegChunk) == (K > chunk));
                                    if (p.refused == kRefuseIntegTile) CHECK(generic == 2 && k.cols_threads == 16);
                                    CHECK(p.second_sweep == ((a.refined || a.qualified) && !p.one_launch));
                                    CHECK(p.need_nb == (a.fine && (!p.one_launch || !a.out_dev)));
                                    CHECK(p.stage_dfrac == (a.fine && !a.out_dev) && (!p.stage_dfrac || p.need_nb));
                                    CHECK(ppb_user ? p.ppb == ppb_user : (p.ppb >= 1 && p.ppb <= 7));
                                    if (p.one_launch) CHECK(!k.generic && D > 1 && W <= chunk && (long)D * W * B <= (1L << 14));
                                    CHECK(p.out_elems == (size_t)(W / K) * P && p.hyp_elems == p.out_elems * (p.one_launch ? D : 1));
                                }
    CHECK(n_plans > 100000);
}

// No planned four-step chunk launches g_cols_inv with more than kMaxGridY rows, or holds more spectra and products than
// generic_chunk_windows' budget: plan_route and plan_caf, 2 ... 32 buoys, every four-step length, the default pair list
// and custom ones, 1 ... 8 bands, groups of 1 ... 8 windows.  The cut is also the tightest: one more group would pass
// the limit (or the ctx's chunk).
static void test_grid_rows() {
    CHECK(cols_inv_grid_rows(560, 1, 120, 1) == 67200 && cols_inv_grid_rows(4800, 1, 28, 2) == 67200);
    CHECK(cols_inv_grid_rows(10, 3, 28, 2) == 420 && cols_inv_grid_rows(10, 0, 28, 0) == 280);
    CHECK(cap_chunk_grid_rows(560, 1, 120, 1) == 546 && cap_chunk_grid_rows(546, 1, 120, 1) == 546);   // 16 buoys: 546 windows
    CHECK(cap_chunk_grid_rows(4096, 1, 28, 1) == 2340 && cap_chunk_grid_rows(4096, 1, 28, 2) == 4096);   // 8 buoys: 2340
    CHECK(cap_chunk_grid_rows(4800, 1, 28, 2) == 4680 && cap_chunk_grid_rows(4800, 1, 28, 7) == 4800);
    CHECK(cap_chunk_grid_rows(64, 1, 70000, 1) == 1 && cap_chunk_grid_rows(64, 1, 70000, 4) == 4);       // one group is never split
    CHECK(cap_chunk_grid_rows(3, 1, 70000, 4) == 3 && cap_chunk_grid_rows(64, 1, 0, 1) == 64);
    long n_plans = 0, n_cut = 0;
    for (int B = 2; B <= 32; ++B)
        for (int logL = 9; logL <= 23; ++logL)
            for (int custom : {0, 1, 2, 3})
                for (int nb = 1; nb <= 8; ++nb)
                    for (int K = 1; K <= 8; ++K) {
                        const long L = 1L << logL, all = (long)B * (B - 1) / 2;
                        const int P = custom == 0 ? (int)all : custom == 1 ? 1 : custom == 2 ? (int)(2 * all + 1) : 2000;
                        RouteCaps k;
                        k.n_cus = 256;  k.n_buoys = B;  k.generic = true;  k.logL = logL;
                        k.small_maxl = logL <= 13 ? 256 : 8192;            // (option small_maxl lowered: the short lengths run four-step)
                        k.g_chunk = (int)generic_chunk_windows(B, L, 1 << 20, kGenericBudgetBytes, 0);
                        RouteCall a;
                        a.n_windows = 8 * 3 * 5 * 7 * 64;  a.n_pairs = P;  a.all_pairs = custom == 0;  a.pairs_given = custom != 0;
                        a.weighted = true;  a.bounded = true;  a.integ = K;  a.n_bands = nb;
                        const RoutePlan p = plan_route(k, a);
                        CafCall ca;
                        ca.n_windows = a.n_windows;  ca.n_pairs = P;  ca.n_dopplers = 5;  ca.integ = K;  ca.n_bands = nb;
                        const CafPlan cp = plan_caf(k, ca);
                        CHECK(p.route == kRouteFourStep);
                        for (int which = 0; which < 2; ++which) {
                            const RouteRefusal refused = which ? cp.refused : p.refused;
                            const long chunk = which ? cp.chunk : p.chunk;
                            ++n_plans;
                            if (refused != kRouteOk) { CHECK(K > 1 || (which && nb > 1)); continue; }
                            CHECK(chunk >= K && chunk % K == 0 && chunk <= k.g_chunk);
                            CHECK(cols_inv_grid_rows(chunk, nb, P, K) <= kMaxGridY);
                            // (a list longer than the default one is not what the ctx's chunk was sized for, and one window
                            // that is over the budget by itself still runs, alone)
                            const long per_win = ((long)B + (nb > 1 ? (long)nb * P : all)) * L * 8;
                            if ((P <= all || nb > 1) && per_win <= kGenericBudgetBytes) CHECK(per_win * chunk <= kGenericBudgetBytes);
                            if (nb == 1) {
                                const long more = chunk + K;
                                CHECK(more > k.g_chunk || cols_inv_grid_rows(more, 1, P, K) > kMaxGridY);
                                n_cut += chunk < k.g_chunk / K * K;
                            }
                        }
                    }
    CHECK(n_plans > 200000 && n_cut > 1000);
    // the whole-window routes' partial round runs four-step too: 255 windows of a 640-pair list
    RouteCaps k;
    k.n_cus = 256;  k.n_buoys = 8;  k.generic = true;  k.logL = 14;  k.g_chunk = 4096;  k.wscr = true;  k.k8 = true;  k.ws_upw = 1;  k.ws_grid = 256;
    RouteCall a;
    a.n_windows = 256 + 40;  a.n_pairs = 640;  a.all_pairs = false;  a.pairs_given = true;
    const RoutePlan p = plan_route(k, a);
    CHECK(p.route == kRouteKWin8 && cols_inv_grid_rows(p.chunk, 1, 640, 1) <= kMaxGridY && p.chunk == 102);
}

int main() {
    test_grid_rows();
    test_route_invariants();
    test_recorded_rows();
    test_recorded_caf_rows();
    test_caf_thresholds();
    test_caf_invariants();
    test_options();
    test_create_args();
    test_request_conversions();
    test_pair_plan();
    test_chunks();
    std::puts("host_plan: all checks passed");
    return 0;
}
