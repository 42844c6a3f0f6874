// host::check_caf_request (radio-mapper_amd/csrc/host_request.hpp) and host::plan_caf (host_plan.hpp) as rmx_caf_batch_bands
// calls them -- every refusal in the entry's order with its text, every extent in n_windows * n_bands * n_pairs slots, the
// per-window bounds once per virtual window, n_bands == 1 giving today's request and plan, the one-launch limits in virtual
// windows, the chunks of the generic routes and the route refusal --, without a GPU: built with
// g++ -fsanitize=address,undefined by tests/test_caf_bands_request_sanitized.py and run directly.  The outputs, the bands
// and the bounds are real arrays of exactly the stated sizes, so a check that read past one would be an AddressSanitizer
// report.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../radio-mapper_amd/csrc/host_request.hpp"

using namespace rmx::host;

static int g_failed = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            ++g_failed;                                                         \
        }                                                                       \
    } while (0)

// five outputs of exactly `slots` elements, each its own allocation
struct Outs {
    std::vector<int32_t> dop, lag;
    std::vector<float> dfrac, frac, peak;
    explicit Outs(size_t slots) : dop(slots), lag(slots), dfrac(slots), frac(slots), peak(slots) {}
};

static const double kGrid[3] = {-0.001, 0.0, 0.001};

// the arguments as rmx_caf_batch_bands and caf_request fill them
static RequestArgs args(Outs& o, int W, int P, int N, const double* bands, int M, int per_window) {
    RequestArgs a;
    a.n_buoys = 4;
    a.n_samples = N;
    a.max_windows = 64;
    a.iq = o.peak.data();   // (never read by the checks)
    a.n_windows = W;
    a.n_pairs = P;
    a.doppler_cps = kGrid;
    a.n_dopplers = 3;
    a.dop_idx = o.dop.data();
    a.dop_frac = o.dfrac.data();
    a.lag_int = o.lag.data();
    a.lag_frac = o.frac.data();
    a.peak = o.peak.data();
    a.grouped = true;
    a.banded = true;
    a.band_cps = bands;
    a.n_bands = M;
    a.band_per_window = per_window;
    return a;
}

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

static int refused(const RequestArgs& a, std::string* err) {
    Request r;
    err->clear();
    return check_caf_request(a, &r, err);
}

static void test_request() {
    const int W = 5, P = 6, N = 256, M = 3;
    const size_t slots = (size_t)W * M * P;
    Outs o(slots);
    Request r;
    std::string err;
    std::vector<double> bands(2 * (size_t)W * M);   // [W][M][2] and not an element more
    for (int k = 0; k < W * M; ++k) {
        bands[2 * k] = -0.3 + 0.01 * k;
        bands[2 * k + 1] = 0.1 + 0.01 * k;
    }
    std::vector<int32_t> lb(2 * (size_t)W * P);     // [W][P][2] and not an element more
    for (int k = 0; k < W * P; ++k) {
        lb[2 * k] = -k - 1;
        lb[2 * k + 1] = k;
    }
    std::vector<int32_t> pl = {0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3};

    // ---- accepted: the band set behind the full band, per-window bounds once per virtual window --------------------------
    RequestArgs a = args(o, W, P, N, bands.data(), M, 1);
    a.lag_bounds = lb.data();
    a.bounds_per_window = 1;
    a.weighting = RMX_WEIGHT_PHAT;
    CHECK(check_caf_request(a, &r, &err) == RMX_OK);
    CHECK(!r.empty && r.n_pairs == P && r.n_bands == M && r.weighted && r.phat && r.band_per_window && r.integ == 1 && r.refine == 0);
    CHECK(r.bins.size() == 2 + 2 * (size_t)W * M && r.bins[0] == -N && r.bins[1] == N - 1);
    CHECK(r.bounded && r.bounds_per_window && r.bound_rows == (long)W * M * P && r.bounds == r.own_bounds.data());
    for (long v = 0; v < (long)W * M; ++v)
        for (int q = 0; q < P; ++q) {
            const long k = (v / M) * P + q;   // the real window's row
            CHECK(r.bounds[2 * (v * P + q)] == -k - 1 && r.bounds[2 * (v * P + q) + 1] == k);
        }
    // shared bounds and a shared band set: nothing replicated
    a = args(o, W, P, N, bands.data(), M, 0);
    a.lag_bounds = lb.data();
    CHECK(check_caf_request(a, &r, &err) == RMX_OK);
    CHECK(r.n_bands == M && !r.band_per_window && r.bins.size() == 2 + 2 * (size_t)M && r.bound_rows == P && r.bounds == lb.data());
    // the default pair list: n_pairs 0 or B (B - 1) / 2
    a = args(o, W, 0, N, bands.data(), M, 1);
    CHECK(check_caf_request(a, &r, &err) == RMX_OK && r.n_pairs == 6);
    a = args(o, W, P, N, bands.data(), M, 1);
    a.pairs = pl.data();
    CHECK(check_caf_request(a, &r, &err) == RMX_OK && r.n_pairs == P);

    // ---- n_bands == 1 IS the single-band request: field for field what rmx_caf_batch_request's arguments give ------------
    {
        Outs o1((size_t)W * P);
        RequestArgs b1 = args(o1, W, P, N, bands.data(), 1, 1);   // reads [W][1][2]
        RequestArgs s1 = b1;
        s1.banded = false;
        s1.n_bands = 0;
        for (unsigned wt : {0u, 1u})
            for (int bounded = 0; bounded < 2; ++bounded) {
                b1.weighting = s1.weighting = wt;
                b1.lag_bounds = s1.lag_bounds = bounded ? lb.data() : nullptr;
                b1.bounds_per_window = s1.bounds_per_window = bounded;
                Request rb, rs;
                CHECK(check_caf_request(b1, &rb, &err) == RMX_OK && check_caf_request(s1, &rs, &err) == RMX_OK);
                CHECK(rb.n_bands == 1 && rs.n_bands == 1 && rb.bins == rs.bins && rb.weighted == rs.weighted && rb.phat == rs.phat);
                CHECK(rb.band_per_window == rs.band_per_window && rb.bounded == rs.bounded && rb.bound_rows == rs.bound_rows);
                CHECK(rb.bounds == rs.bounds && rb.own_bounds.empty() && rs.own_bounds.empty() && rb.n_pairs == rs.n_pairs);
            }
    }

    // ---- every refusal, in the entry's order, with its text ----------------------------------------------------------------
    // one call that is wrong in every way: each repair uncovers the next check
    std::vector<double> bad_bands = bands;
    bad_bands[2 * (1 * M + 2)] = 0.4;   // window 1, band 2: lo > hi
    bad_bands[2 * (1 * M + 2) + 1] = 0.3;
    std::vector<int32_t> bad_lb = lb;
    bad_lb[2 * (2 * P + 4)] = 9;        // window 2, pair 4
    bad_lb[2 * (2 * P + 4) + 1] = 8;
    std::vector<int32_t> bad_pl = pl;
    bad_pl[7] = 4;                      // pair 3 = (1, 4): no such buoy
    a = args(o, 65, P, N, nullptr, 0, 1);
    a.n_dopplers = 0;
    a.pairs = bad_pl.data();
    a.weighting = 7;
    a.lag_bounds = bad_lb.data();
    a.bounds_per_window = 1;
    a.dop_frac = o.peak.data();
    a.flags = RMX_OUT_DEVICE;
    std::vector<char> odd(4 * slots + 8);
    a.lag_frac = reinterpret_cast<float*>(odd.data() + 2);
    // 1. the head: a NULL buffer (band_cps included), a misaligned device pointer, n_dopplers
    CHECK(refused(a, &err) == RMX_E_INVAL && err == "NULL buffer");
    a.band_cps = bad_bands.data();
    {
        RequestArgs n = a;
        n.doppler_cps = nullptr;
        CHECK(refused(n, &err) == RMX_E_INVAL && err == "NULL buffer");
        n = a;
        n.dop_idx = nullptr;
        CHECK(refused(n, &err) == RMX_E_INVAL && err == "NULL buffer");
    }
    CHECK(refused(a, &err) == RMX_E_INVAL && has(err, "lag_frac is a device pointer 2 bytes past a multiple of 4"));
    a.lag_frac = o.frac.data();
    a.flags = 0;
    CHECK(refused(a, &err) == RMX_E_INVAL && err == "n_dopplers 0 not in 1..4096");
    a.n_dopplers = 4097;
    CHECK(refused(a, &err) == RMX_E_INVAL && err == "n_dopplers 4097 not in 1..4096");
    a.n_dopplers = 3;
    // 2. n_bands
    for (int m : {0, -1, 65}) {
        a.n_bands = m;
        char want[48];
        std::snprintf(want, sizeof want, "n_bands %d not in 1..64", m);
        CHECK(refused(a, &err) == RMX_E_INVAL && err == want);
    }
    a.n_bands = M;
    // 3. the batch shape and the pair list
    CHECK(refused(a, &err) == RMX_E_INVAL && err == "n_windows 65 not in 0..max_windows=64");
    a.n_windows = -1;
    CHECK(refused(a, &err) == RMX_E_INVAL && has(err, "n_windows -1 not in"));
    a.n_windows = W;
    a.n_pairs = -2;
    CHECK(refused(a, &err) == RMX_E_INVAL && err == "n_pairs -2 < 0");
    a.n_pairs = P;
    CHECK(refused(a, &err) == RMX_E_INVAL && err == "pair 3 = (1,4) out of range for 4 buoys");
    a.pairs = nullptr;
    a.n_pairs = 5;
    CHECK(refused(a, &err) == RMX_E_INVAL && has(err, "pairs == NULL needs n_pairs == 0 or 6, got 5"));
    a.n_pairs = P;
    // 4. the weighting and the bands: the window and the band index
    CHECK(refused(a, &err) == RMX_E_INVAL && has(err, "unknown weighting 7"));
    a.weighting = RMX_WEIGHT_PHAT;
    CHECK(refused(a, &err) == RMX_E_INVAL && has(err, "band 2 of window 1: [0.4, 0.3] is not an interval inside [-0.5, 0.5]"));
    {
        RequestArgs s = a;   // the shared form says so, and a band without a bin
        s.band_per_window = 0;
        std::vector<double> sh = {-0.2, 0.1, 0.1 / N, 0.2 / N, 0.2, 0.3};
        s.band_cps = sh.data();
        CHECK(refused(s, &err) == RMX_E_INVAL);
        CHECK(has(err, "band 1 of window 0 (one band set shared by every window)") && has(err, "keeps no bin of the 512-point transform"));
    }
    a.band_cps = bands.data();
    // 5. the bounds
    CHECK(refused(a, &err) == RMX_E_INVAL && has(err, "lag_bounds of window 2, pair 4: [9, 8] is not an interval inside [-255, 255]"));
    a.lag_bounds = lb.data();
    // 6. dop_frac over another output: every extent W * M * P elements
    CHECK(refused(a, &err) == RMX_E_INVAL && has(err, "dop_frac overlaps peak") && has(err, "its 90 floats need a buffer of their own"));
    {
        std::vector<float> slab(2 * slots, 0.0f);   // dop_idx | dop_frac back to back: W * M * P elements each and not one more
        a.dop_idx = reinterpret_cast<int32_t*>(slab.data());
        a.dop_frac = slab.data() + slots;
        CHECK(check_caf_request(a, &r, &err) == RMX_OK);
        a.dop_frac = slab.data() + slots - 1;
        CHECK(refused(a, &err) == RMX_E_INVAL && has(err, "dop_frac overlaps dop_idx"));
        a.dop_idx = o.dop.data();
        a.dop_frac = nullptr;   // not computed: nothing to overlap
        CHECK(check_caf_request(a, &r, &err) == RMX_OK);
    }
    // an empty batch: RMX_OK, nothing to do -- behind the head and n_bands, in front of the bands
    a = args(o, 0, P, N, bad_bands.data(), M, 1);
    CHECK(check_caf_request(a, &r, &err) == RMX_OK && r.empty);
    a = args(o, W, 0, N, bad_bands.data(), M, 1);
    a.pairs = pl.data();
    CHECK(check_caf_request(a, &r, &err) == RMX_OK && r.empty);
    a.n_bands = 0;
    CHECK(refused(a, &err) == RMX_E_INVAL && has(err, "n_bands 0"));
}

static RouteCaps caps4096() {
    RouteCaps k;
    k.n_cus = 256;
    k.n_buoys = 3;
    k.generic = false;
    k.chunk_windows = 4096;
    return k;
}
static RouteCaps caps_generic(int logL, int g_chunk) {
    RouteCaps k;
    k.n_cus = 256;
    k.n_buoys = 3;
    k.generic = true;
    k.logL = logL;
    k.logL1 = logL / 2;
    k.logL2 = logL - logL / 2;
    k.g_chunk = g_chunk;
    return k;
}
static CafCall call(int W, int P, int D, int M) {
    CafCall a;
    a.n_windows = W;
    a.n_pairs = P;
    a.n_dopplers = D;
    a.n_bands = M;
    return a;
}
static bool same_plan(const CafPlan& x, const CafPlan& y) {
    return x.one_launch == y.one_launch && x.ppb == y.ppb && x.chunk == y.chunk && x.refused == y.refused && x.out_elems == y.out_elems &&
           x.hyp_elems == y.hyp_elems && x.need_nb == y.need_nb && x.stage_dfrac == y.stage_dfrac && x.second_sweep == y.second_sweep;
}

static void test_plan() {
    // ---- n_bands == 1 (and the default) gives the fields of today: out = W P, hyp = D W P in one launch ------------------
    for (int W : {1, 8, 64, 5000})
        for (int D : {1, 5, 21}) {
            const RouteCaps k = caps4096();
            CafCall a = call(W, 3, D, 1), d = a;
            d.n_bands = 1;
            a.fine = d.fine = true;
            const CafPlan p = plan_caf(k, a);
            CHECK(same_plan(p, plan_caf(k, d)));
            CHECK(p.out_elems == (size_t)W * 3 && p.hyp_elems == (p.one_launch ? (size_t)D * W * 3 : (size_t)W * 3));
            CHECK(p.one_launch == (D > 1 && W <= 4096 && (size_t)D * W * 3 * kSpecBytes4096 <= ((size_t)1 << 30) && (long)D * W < (1L << 20)));
            CHECK(p.chunk == 4096 && p.refused == kRouteOk);
        }
    // ---- M > 1: slots, the per-hypothesis arrays, and ppb sized to D W M work items ------------------------------------------
    {
        const RouteCaps k = caps4096();
        const CafPlan p = plan_caf(k, call(8, 3, 21, 4));
        CHECK(p.one_launch && p.out_elems == 8u * 4 * 3 && p.hyp_elems == 21u * 8 * 4 * 3 && p.refused == kRouteOk);
        int ppb = 0;
        (void)split_cost4096(k.n_cus, k.n_buoys, 3, 8L * 21 * 4, 0, &ppb);
        CHECK(p.ppb == ppb);
        const CafPlan s = plan_caf(k, call(5000, 3, 21, 4));   // over chunks: one hypothesis' slots
        CHECK(!s.one_launch && s.out_elems == 5000u * 4 * 3 && s.hyp_elems == s.out_elems && s.chunk == 4096);
        (void)split_cost4096(k.n_cus, k.n_buoys, 3, 5000L * 4, 0, &ppb);
        CHECK(s.ppb == ppb);
        RouteCaps u = k;
        u.ppb_user = 3;
        CHECK(plan_caf(u, call(8, 3, 21, 4)).ppb == 3);
    }
    // ---- the one-launch limits count VIRTUAL windows: D W M just below and at 2^20; the spectra bound does not move ----------
    {
        // the 1 GiB bound: D W B spectra of 64 KiB, whatever M.  B = 2: D W <= 8192
        RouteCaps k = caps4096();
        k.n_buoys = 2;
        k.chunk_windows = 1 << 20;
        for (int M : {1, 2, 64}) {
            CHECK(plan_caf(k, call(4096, 1, 2, M)).one_launch);     // D W = 8192: exactly 1 GiB (D W M at most 2^19)
            CHECK(!plan_caf(k, call(4097, 1, 2, M)).one_launch);    // one window more: past it
        }
        // The virtual windows: with two buoys or more the spectra bound bites first (D W <= 8192 and M <= 64 give at most
        // 2^19), so the limit itself is reached on the plan's arithmetic alone, with one buoy: D W = 16384 spectra = 1 GiB
        k.n_buoys = 1;
        k.chunk_windows = 8;
        CHECK((long)4096 * 4 * 63 < (1L << 20) && (long)4096 * 4 * 64 == (1L << 20));
        CHECK(plan_caf(k, call(4, 1, 4096, 63)).one_launch);        // 2^20 - 16384 virtual windows: one launch
        CHECK(!plan_caf(k, call(4, 1, 4096, 64)).one_launch);       // at 2^20: the sweep
        CHECK(plan_caf(k, call(4, 1, 4096, 1)).one_launch);         // M = 1 is far below it
        const CafPlan p = plan_caf(k, call(4, 1, 4096, 63));
        CHECK(p.hyp_elems == (size_t)4096 * 4 * 63 && p.out_elems == 4u * 63);
        const CafPlan q = plan_caf(k, call(4, 1, 4096, 64));
        CHECK(q.hyp_elems == q.out_elems && q.out_elems == 4u * 64 && q.chunk == 8);
        CHECK(!plan_caf(k, call(9, 1, 5, 2)).one_launch);           // more windows than one chunk
    }
    // ---- N = 4096 in chunks: chunk_windows, cut so that a chunk's virtual windows stay under the pair grid's bound ----------
    {
        RouteCaps k = caps4096();
        k.chunk_windows = 8;
        CHECK(plan_caf(k, call(64, 3, 21, 8)).chunk == 8);
        k.chunk_windows = 1 << 20;
        const CafPlan p = plan_caf(k, call(64, 3, 1, 64));
        CHECK(p.chunk == (int)(((1L << 20) - 1) / 64) && (long)p.chunk * 64 < (1L << 20) && p.refused == kRouteOk);
        CHECK(plan_caf(k, call(64, 3, 1, 1)).chunk == 1 << 20);
    }
    // ---- the generic routes: plan_bands' chunk for M bands, the per-slot buffers' cap ----------------------------------------
    for (int logL : {9, 14})   // N = 256 (small) and N = 8192 (four-step)
        for (int g_chunk : {2, 64, 4096})
            for (int M : {1, 2, 3, 64}) {
                const RouteCaps k = caps_generic(logL, g_chunk);
                const bool four = (1L << logL) > k.small_maxl;
                const CafPlan p = plan_caf(k, call(5, 3, 5, M));
                const long want = M > 1 ? plan_bands(g_chunk, 5, M, 3, 3, 1L << logL, four, 0, 0, 0).chunk : g_chunk;
                CHECK(p.chunk == want && p.refused == kRouteOk && !p.one_launch);
                CHECK((long)p.chunk * M <= (M > 1 ? kGenericMaxChunk : (long)g_chunk * M) && p.chunk >= 1);
                CHECK(p.out_elems == 5u * M * 3 && p.hyp_elems == p.out_elems);
                if (four && M > 1) CHECK((long)p.chunk * M * 3 <= kMaxGridY);
            }
    CHECK(plan_caf(caps_generic(9, 2), call(5, 3, 5, 3)).chunk == 2);          // a small chunk is not shrunk further
    CHECK(plan_caf(caps_generic(9, 4096), call(5, 3, 5, 64)).chunk == 64);     // 4096 virtual windows
    CHECK(plan_caf(caps_generic(14, 4096), call(5, 3, 5, 64)).chunk == 64);
    // ---- the route refusal: a window whose own M * P slots no chunk holds (one grid row per slot of the column pass) ----------
    {
        RouteCaps k = caps_generic(14, 64);
        k.n_buoys = 64;                                     // 2016 pairs
        CHECK(plan_caf(k, call(2, 2016, 5, 32)).refused == kRouteOk);       // 64512 slots per window
        const CafPlan p = plan_caf(k, call(2, 2016, 5, 33));                // 66528 > 65535
        CHECK(p.refused == kRefuseBandsChunk && p.chunk == 0);
        CHECK(plan_caf(k, call(2, 2016, 5, 1)).refused == kRouteOk);        // never without bands
        const RouteCaps s = caps_generic(9, 64);                            // the small route has no such grid
        RouteCaps s64 = s;
        s64.n_buoys = 64;
        CHECK(plan_caf(s64, call(2, 2016, 5, 64)).refused == kRouteOk);
        RouteCaps big = caps_generic(22, 4);                                // L = 4 Mi bins: 32 GiB hold 1024 product slots
        CHECK(plan_caf(big, call(2, 3, 5, 64)).refused == kRouteOk);        // 192 slots + 3 spectra
        big.n_buoys = 64;
        CHECK(plan_caf(big, call(2, 2016, 5, 2)).refused == kRefuseBandsChunk);   // 4032 slots of 32 MiB each
    }
}

int main() {
    test_request();
    test_plan();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
