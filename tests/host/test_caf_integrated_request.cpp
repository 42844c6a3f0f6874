// host::check_groups and host::check_caf_request (radio-mapper_amd/csrc/host_request.hpp) as rmx_caf_batch_integrated calls
// them -- the group count, then per-window bands, per-GROUP bounds, every output extent in G * n_pairs slots, refine,
// quality --, without a GPU: built with g++ -fsanitize=address,undefined by tests/test_caf_integrated_cpu.py and run
// directly.  The outputs and the bounds are real arrays of exactly the stated sizes, so a check that read past one --
// n_windows rows of bounds instead of G, n_windows * n_pairs slots instead of G * n_pairs -- would be an AddressSanitizer
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

// six outputs of exactly `slots` elements (quality: 4 x), each its own allocation
struct Outs {
    std::vector<int32_t> dop, lag;
    std::vector<float> dfrac, frac, peak, quality;
    explicit Outs(size_t slots) : dop(slots), lag(slots), dfrac(slots), frac(slots), peak(slots), quality(4 * slots) {}
};

static RequestArgs args(Outs& o, int W, int P, int N, int K) {
    RequestArgs a;
    a.n_buoys = 4;
    a.n_samples = N;
    a.max_windows = 64;
    a.iq = o.peak.data();   // (never read by the checks)
    a.n_windows = W;
    a.n_pairs = P;
    a.lag_int = o.lag.data();
    a.lag_frac = o.frac.data();
    a.peak = o.peak.data();
    a.quality = o.quality.data();
    a.refine = 8;
    a.grouped = true;
    a.integrate = K;
    return a;
}

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

int main() {
    const int W = 12, P = 6, N = 256, K = 4, G = W / K;
    const size_t slots = (size_t)G * P;
    Outs o(slots);
    Request r;
    std::string err;

    // ---- the group count: the values in the text ------------------------------------------------------------------------
    CHECK(check_groups(K, W, &err) == RMX_OK);
    CHECK(check_groups(1, W, &err) == RMX_OK && check_groups(W, W, &err) == RMX_OK);
    for (int k : {0, -1, -7}) {
        err.clear();
        CHECK(check_groups(k, W, &err) == RMX_E_INVAL);
        char want[40];
        std::snprintf(want, sizeof want, "integrate = %d:", k);
        CHECK(has(err, want));
    }
    err.clear();
    CHECK(check_groups(5, W, &err) == RMX_E_INVAL && has(err, "n_windows = 12 is not a positive multiple of integrate = 5"));
    CHECK(check_groups(24, W, &err) == RMX_E_INVAL && has(err, "n_windows = 12") && has(err, "integrate = 24"));
    CHECK(check_groups(2, 0, &err) == RMX_E_INVAL && has(err, "n_windows = 0"));

    // ---- accepted: K handed on, the outputs G * P slots, without bounds the full interval per pair, one row ------------
    RequestArgs a = args(o, W, P, N, K);
    CHECK(check_caf_request(a, o.dop.data(), o.dfrac.data(), &r, &err) == RMX_OK);
    CHECK(r.integ == K && r.refine == 8 && r.n_pairs == P && !r.weighted);
    CHECK(r.bounded && r.bound_rows == P && !r.bounds_per_window && r.bounds == r.own_bounds.data());
    for (int q = 0; q < P; ++q) CHECK(r.bounds[2 * q] == -(N - 1) && r.bounds[2 * q + 1] == N - 1);
    // one window per group is the ungrouped request: nothing carried
    a = args(o, G, P, N, 1);
    CHECK(check_caf_request(a, o.dop.data(), o.dfrac.data(), &r, &err) == RMX_OK && r.integ == 1 && !r.bounded);

    // ---- per-group bounds: exactly G * P rows are read and handed on, to the last row -----------------------------------
    {
        std::vector<int32_t> lb(2 * slots);   // [G][P][2] and not an element more
        for (size_t k = 0; k < slots; ++k) {
            lb[2 * k] = -(int)k - 1;
            lb[2 * k + 1] = (int)k;
        }
        a = args(o, W, P, N, K);
        a.lag_bounds = lb.data();
        a.bounds_per_window = 1;
        CHECK(check_caf_request(a, o.dop.data(), o.dfrac.data(), &r, &err) == RMX_OK);
        CHECK(r.bounded && r.bounds_per_window && r.bound_rows == (long)slots && r.bounds == lb.data());
        long sum = 0;
        for (long k = 0; k < 2 * r.bound_rows; ++k) sum += r.bounds[k];   // the staging copy's extent
        CHECK(sum == -(long)slots);
        CHECK(r.bounds[2 * (slots - 1)] == -(int)slots && r.bounds[2 * (slots - 1) + 1] == (int)slots - 1);
        // a bad interval in the LAST row of the last group: the text says "group"
        lb[2 * (slots - 1)] = 9;
        lb[2 * (slots - 1) + 1] = 8;
        err.clear();
        CHECK(check_caf_request(a, o.dop.data(), o.dfrac.data(), &r, &err) == RMX_E_INVAL);
        CHECK(has(err, "lag_bounds of group 2, pair 5") && !has(err, "window"));
        // shared bounds: [P][2]
        std::vector<int32_t> sh(2 * P, 0);
        sh[3] = -1;   // pair 1: [0, -1]
        a.lag_bounds = sh.data();
        a.bounds_per_window = 0;
        err.clear();
        CHECK(check_caf_request(a, o.dop.data(), o.dfrac.data(), &r, &err) == RMX_E_INVAL && has(err, "lag_bounds of group -1, pair 1"));
        sh[3] = 0;
        CHECK(check_caf_request(a, o.dop.data(), o.dfrac.data(), &r, &err) == RMX_OK && r.bound_rows == P && r.bounded);
    }

    // ---- the bands stay per WINDOW: W rows are read, and a bad one names its real window --------------------------------
    {
        std::vector<double> bands(2 * (size_t)W);   // [W][2] and not an element more
        for (int w = 0; w < W; ++w) {
            bands[2 * w] = -0.25;
            bands[2 * w + 1] = 0.25 + 0.01 * w;
        }
        a = args(o, W, P, N, K);
        a.band_cps = bands.data();
        a.band_per_window = 1;
        CHECK(check_caf_request(a, o.dop.data(), o.dfrac.data(), &r, &err) == RMX_OK);
        CHECK(r.weighted && r.band_per_window && r.bins.size() == 2 * (size_t)W);
        bands[2 * (W - 1)] = 0.4;   // lo > hi in the last window of the last group
        err.clear();
        CHECK(check_caf_request(a, o.dop.data(), o.dfrac.data(), &r, &err) == RMX_E_INVAL && has(err, "band of window 11"));
    }

    // ---- the extents are G * P slots: an array that starts right behind another's G * P elements does not overlap it ------
    {
        std::vector<float> slab(6 * slots, 0.0f);   // dop_idx | dop_frac, and quality behind them: W * P slots would collide
        int32_t* dop = reinterpret_cast<int32_t*>(slab.data());
        a = args(o, W, P, N, K);
        a.quality = slab.data() + 2 * slots;
        CHECK(check_caf_request(a, dop, slab.data() + slots, &r, &err) == RMX_OK);
        err.clear();
        CHECK(check_caf_request(a, dop, slab.data() + slots - 1, &r, &err) == RMX_E_INVAL);
        CHECK(has(err, "dop_frac overlaps dop_idx") && has(err, "its 18 floats"));
        a.quality = slab.data() + 2 * slots - 1;
        err.clear();
        CHECK(check_caf_request(a, dop, slab.data() + slots, &r, &err) == RMX_E_INVAL);
        CHECK(has(err, "quality overlaps dop_frac") && has(err, "18 x 4 floats"));
    }

    // ---- the order: weighting and bands, bounds, dop_frac's overlap, refine, quality's overlap, quality's alignment -----
    {
        a = args(o, W, P, N, K);
        a.weighting = 7;
        a.refine = 3;
        a.quality = o.peak.data();
        std::vector<int32_t> lb(2 * P, 0);
        lb[2] = 5;
        lb[3] = 4;
        a.lag_bounds = lb.data();
        CHECK(check_caf_request(a, o.dop.data(), o.peak.data(), &r, &err) == RMX_E_INVAL && has(err, "unknown weighting 7"));
        a.weighting = RMX_WEIGHT_PHAT;
        CHECK(check_caf_request(a, o.dop.data(), o.peak.data(), &r, &err) == RMX_E_INVAL && has(err, "lag_bounds of group -1, pair 1"));
        a.lag_bounds = nullptr;
        CHECK(check_caf_request(a, o.dop.data(), o.peak.data(), &r, &err) == RMX_E_INVAL && has(err, "dop_frac overlaps peak"));
        CHECK(check_caf_request(a, o.dop.data(), o.dfrac.data(), &r, &err) == RMX_E_INVAL && has(err, "refine = 3:"));
        a.refine = 4;
        CHECK(check_caf_request(a, o.dop.data(), o.dfrac.data(), &r, &err) == RMX_E_INVAL && has(err, "quality overlaps peak"));
        std::vector<char> own(4 * slots * sizeof(float) + 8);
        a.quality = reinterpret_cast<float*>(own.data() + 2);
        a.flags = RMX_OUT_DEVICE;
        CHECK(check_caf_request(a, o.dop.data(), o.dfrac.data(), &r, &err) == RMX_E_INVAL);
        CHECK(has(err, "quality is a device pointer 2 bytes past a multiple of 4"));
        a.flags = 0;
        CHECK(check_caf_request(a, o.dop.data(), o.dfrac.data(), &r, &err) == RMX_OK && r.integ == K && r.refine == 4);
    }

    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
