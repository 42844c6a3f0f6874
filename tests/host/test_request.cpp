// The checked request of the correlation and Doppler-search entries (radio-mapper_amd/csrc/host_request.hpp) under
// AddressSanitizer + UBSan.  Built and run by tests/test_request_sanitized.py:  g++ -std=c++17 -O1 -g
// -fsanitize=address,undefined -fno-sanitize-recover=all -o ... tests/host/test_request.cpp ; exit code 0 = every check
// passed and neither sanitizer reported anything.
// Every caller array is a heap block of exactly the size include/rmx.h states for the call (a std::vector built with
// that size), so a check that reads one row too far is a sanitizer report.  The refusal texts are those
// tests/test_gpu_bands.py, test_gpu_bands_quality.py, test_gpu_quality.py and test_gpu_caf_request.py look for.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../radio-mapper_amd/csrc/host_request.hpp"

using namespace rmx::host;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

static const int B = 3, N = 16, MAXW = 4, W = 4, M = 3, P = 3;
static const double NaN = std::numeric_limits<double>::quiet_NaN();

// the four outputs of one call: [slots] each, quality [slots][4]
struct Outs {
    std::vector<int32_t> lag_int;
    std::vector<float> lag_frac, peak, quality;
    explicit Outs(size_t slots) : lag_int(slots), lag_frac(slots), peak(slots), quality(4 * slots) {}
};
static std::vector<float> g_iq(1);   // never read by a check: only its address counts

// ---- the eight entries, as rmx_hip.hip fills the arguments ---------------------------------------------------------------
static RequestArgs plain(Outs& o, int n_windows = W, const int32_t* pairs = nullptr, int n_pairs = P) {
    RequestArgs a;
    a.n_buoys = B;
    a.n_samples = N;
    a.max_windows = MAXW;
    a.iq = g_iq.data();
    a.n_windows = n_windows;
    a.pairs = pairs;
    a.n_pairs = n_pairs;
    a.lag_int = o.lag_int.data();
    a.lag_frac = o.lag_frac.data();
    a.peak = o.peak.data();
    return a;
}
static RequestArgs bounded(RequestArgs a, const std::vector<int32_t>* lb, int per_window) {
    a.bounds_required = true;
    a.lag_bounds = lb ? lb->data() : nullptr;
    a.bounds_per_window = per_window;
    return a;
}
static RequestArgs weighted(RequestArgs a, const std::vector<double>* bands, int per_window, unsigned weighting,
                            const std::vector<int32_t>* lb = nullptr, int lb_per_window = 0) {
    a.band_cps = bands ? bands->data() : nullptr;
    a.band_per_window = per_window;
    a.weighting = weighting;
    a.lag_bounds = lb ? lb->data() : nullptr;
    a.bounds_per_window = lb_per_window;
    return a;
}
static RequestArgs grouped(RequestArgs a, int integrate, int refine = 0, float* quality = nullptr) {   // _integrated, _refined, _quality
    a.grouped = true;
    a.integrate = integrate;
    a.refine = refine;
    a.quality = quality;
    return a;
}
static RequestArgs banded(RequestArgs a, int n_bands, int refine = 0, float* quality = nullptr) {      // _bands, _bands_quality
    a.banded = true;
    a.n_bands = n_bands;
    a.refine = refine;
    a.quality = quality;
    return a;
}

static void refused(const RequestArgs& a, const char* text, int line) {
    Request r;
    std::string err;
    const int rc = check_request(a, &r, &err);
    if (rc != RMX_E_INVAL || err != text) {
        std::fprintf(stderr, "line %d: rc %d, text \"%s\"\n  wanted RMX_E_INVAL, \"%s\"\n", line, rc, err.c_str(), text);
        std::exit(1);
    }
}
#define REFUSED(a, text) refused((a), (text), __LINE__)
static Request accepted(const RequestArgs& a, int line) {
    Request r;
    std::string err;
    const int rc = check_request(a, &r, &err);
    if (rc != RMX_OK) {
        std::fprintf(stderr, "line %d: rc %d, text \"%s\", wanted RMX_OK\n", line, rc, err.c_str());
        std::exit(1);
    }
    return r;
}
#define ACCEPTED(a) accepted((a), __LINE__)

// ---- arrays of exactly the stated size -----------------------------------------------------------------------------------
static std::vector<double> bands_of(int rows, double lo = -0.25, double hi = 0.25) {
    std::vector<double> b((size_t)(2 * rows));
    for (int r = 0; r < rows; ++r) {
        b[2 * r] = lo;
        b[2 * r + 1] = hi;
    }
    return b;
}
static std::vector<int32_t> bounds_of(int rows, int lo = -3, int hi = 3) {
    std::vector<int32_t> b((size_t)(2 * rows));
    for (int r = 0; r < rows; ++r) {
        b[2 * r] = lo;
        b[2 * r + 1] = hi;
    }
    return b;
}
static const char kNull[] = "NULL buffer";
static const char kWeighting[] = "unknown weighting 7 (RMX_WEIGHT_NONE = 0, RMX_WEIGHT_PHAT = 1)";
static const char kRefine[] = "refine = 3: the fine grid is 1 / U samples with U one of 0 (none), 2, 4, 8, 16";

// ---- 1. every refusal of every entry family, with its text ------------------------------------------------------------------
static void test_refusal_texts() {
    Outs o((size_t)W * P), om((size_t)W * M * P);
    const std::vector<double> band1 = bands_of(1), bandW = bands_of(W), set = bands_of(M), setW = bands_of(W * M);
    const std::vector<int32_t> lbP = bounds_of(P), lbWP = bounds_of(W * P), lbG = bounds_of(2 * P);
    // a NULL buffer: each of the four every entry takes, lag_bounds of the bounded entry, band_cps of the banded ones
    for (int k = 0; k < 4; ++k) {
        RequestArgs a = plain(o);
        if (k == 0) a.iq = nullptr;
        if (k == 1) a.lag_int = nullptr;
        if (k == 2) a.lag_frac = nullptr;
        if (k == 3) a.peak = nullptr;
        REFUSED(a, kNull);
        REFUSED(weighted(a, &band1, 0, RMX_WEIGHT_PHAT), kNull);
        REFUSED(grouped(a, 2, 4, o.quality.data()), kNull);
        REFUSED(banded(weighted(a, &set, 0, 0), M, 4, om.quality.data()), kNull);
    }
    REFUSED(bounded(plain(o), nullptr, 0), kNull);
    REFUSED(banded(weighted(plain(om), nullptr, 0, 0), M), kNull);
    REFUSED(banded(weighted(plain(om), nullptr, 1, 0), M, 4, om.quality.data()), kNull);
    // the grouped entries: integrate, the group count
    REFUSED(grouped(plain(o), 0), "integrate = 0: at least one window per group");
    REFUSED(grouped(plain(o), -2, 4), "integrate = -2: at least one window per group");
    REFUSED(grouped(plain(o), 3, 0, o.quality.data()), "n_windows = 4 is not a positive multiple of integrate = 3");
    REFUSED(grouped(plain(o, 0), 1), "n_windows = 0 is not a positive multiple of integrate = 1");
    REFUSED(grouped(plain(o, -4), 2), "n_windows = -4 is not a positive multiple of integrate = 2");
    // n_bands
    REFUSED(banded(weighted(plain(om), &set, 0, 0), 0), "n_bands 0 not in 1..64");
    REFUSED(banded(weighted(plain(om), &set, 0, 0), 65, 4, om.quality.data()), "n_bands 65 not in 1..64");
    REFUSED(banded(weighted(plain(om), &set, 0, 0), -1), "n_bands -1 not in 1..64");
    // the weighting, through every family that takes one
    REFUSED(weighted(plain(o), nullptr, 0, 7), kWeighting);
    REFUSED(weighted(plain(o), &band1, 0, 7), kWeighting);
    REFUSED(grouped(weighted(plain(o), &bandW, 1, 7), 2), kWeighting);
    REFUSED(banded(weighted(plain(om), &set, 0, 7), M), kWeighting);
    REFUSED(banded(weighted(plain(om), &setW, 1, 7), M, 2, om.quality.data()), kWeighting);
    REFUSED(weighted(plain(o), nullptr, 0, 2), "unknown weighting 2 (RMX_WEIGHT_NONE = 0, RMX_WEIGHT_PHAT = 1)");
    // n_windows in front of the bands (a weighted call), and as the batch shape (a plain one)
    REFUSED(weighted(plain(o, W + 1), &band1, 0, 0), "n_windows 5 not in 0..max_windows=4");
    REFUSED(weighted(plain(o, -1), nullptr, 0, RMX_WEIGHT_PHAT), "n_windows -1 not in 0..max_windows=4");
    REFUSED(banded(weighted(plain(om, W + 1), &set, 0, 0), M), "n_windows 5 not in 0..max_windows=4");
    REFUSED(plain(o, W + 1), "n_windows 5 not in 0..max_windows=4");
    REFUSED(bounded(plain(o, -1), &lbP, 0), "n_windows -1 not in 0..max_windows=4");
    // a band: the single-band entries name the window, the banded ones the band and the window
    struct { double lo, hi; const char* why; } bad[5] = {
        {0.5, 0.5, "[0.5, 0.5] keeps no bin of the 32-point transform"},
        {NaN, 0.1, "[nan, 0.1] is not an interval inside [-0.5, 0.5] cycles per sample"},
        {0.2, 0.1, "[0.2, 0.1] is not an interval inside [-0.5, 0.5] cycles per sample"},
        {-0.6, 0.1, "[-0.6, 0.1] is not an interval inside [-0.5, 0.5] cycles per sample"},
        {1e-09, 2e-09, "[1e-09, 2e-09] keeps no bin of the 32-point transform"}};
    for (const auto& b : bad) {
        std::vector<double> one = band1, per = bandW, s = set, sw = setW;
        one[0] = b.lo; one[1] = b.hi;
        per[2 * 2] = b.lo; per[2 * 2 + 1] = b.hi;                            // window 2
        s[2 * 1] = b.lo; s[2 * 1 + 1] = b.hi;                                // band 1
        sw[2 * (2 * M + 1)] = b.lo; sw[2 * (2 * M + 1) + 1] = b.hi;          // band 1 of window 2
        const std::string t_one = std::string("band of window 0 (one band shared by every window): ") + b.why;
        const std::string t_per = std::string("band of window 2: ") + b.why;
        const std::string t_s = std::string("band 1 of window 0 (one band set shared by every window): ") + b.why;
        const std::string t_sw = std::string("band 1 of window 2: ") + b.why;
        REFUSED(weighted(plain(o), &one, 0, 0), t_one.c_str());
        REFUSED(weighted(plain(o), &per, 1, RMX_WEIGHT_PHAT), t_per.c_str());
        REFUSED(grouped(weighted(plain(o), &per, 1, 0), 2, 4, o.quality.data()), t_per.c_str());
        REFUSED(banded(weighted(plain(om), &s, 0, 0), M), t_s.c_str());
        REFUSED(banded(weighted(plain(om), &sw, 1, RMX_WEIGHT_PHAT), M, 4, om.quality.data()), t_sw.c_str());
        // n_bands == 1 is the weighted request, refused in the banded entry's words: band 0 of window r
        const std::string t_b1 = std::string("band 0 of window 2: ") + b.why;
        const std::string t_b1s = std::string("band 0 of window 0 (one band set shared by every window): ") + b.why;
        REFUSED(banded(weighted(plain(o), &per, 1, 0), 1), t_b1.c_str());
        REFUSED(banded(weighted(plain(o), &one, 0, 0), 1, 4, o.quality.data()), t_b1s.c_str());
    }
    // the batch shape
    const std::vector<int32_t> two = {0, 1, 1, 2};
    REFUSED(plain(o, W, nullptr, 2), "pairs == NULL needs n_pairs == 0 or 3, got 2");
    REFUSED(banded(weighted(plain(om, W, nullptr, 2), &set, 0, 0), M, 4, om.quality.data()), "pairs == NULL needs n_pairs == 0 or 3, got 2");
    REFUSED(plain(o, W, two.data(), -1), "n_pairs -1 < 0");
    REFUSED(grouped(weighted(plain(o, W, two.data(), -2), &band1, 0, 0), 2), "n_pairs -2 < 0");
    // the bounds: shared ("window -1"), per window, per group
    for (int k = 0; k < 3; ++k) {
        const int lo = k == 0 ? -N : k == 1 ? 0 : 5, hi = k == 0 ? 0 : k == 1 ? N : 4;
        char tail[96], text[192];
        std::snprintf(tail, sizeof tail, "pair 2: [%d, %d] is not an interval inside [-15, 15]", lo, hi);
        std::vector<int32_t> sh = lbP, pw = lbWP, pg = lbG;
        sh[2 * 2] = lo; sh[2 * 2 + 1] = hi;
        pw[2 * (1 * P + 2)] = lo; pw[2 * (1 * P + 2) + 1] = hi;              // window (group) 1, pair 2
        pg[2 * (1 * P + 2)] = lo; pg[2 * (1 * P + 2) + 1] = hi;
        std::snprintf(text, sizeof text, "lag_bounds of window -1, %s", tail);
        REFUSED(bounded(plain(o), &sh, 0), text);
        REFUSED(weighted(plain(o), &band1, 0, RMX_WEIGHT_PHAT, &sh, 0), text);
        REFUSED(banded(weighted(plain(om), &set, 0, 0, &sh, 0), M), text);
        std::snprintf(text, sizeof text, "lag_bounds of window 1, %s", tail);
        REFUSED(bounded(plain(o), &pw, 1), text);
        REFUSED(grouped(weighted(plain(o), nullptr, 0, 0, &pw, 1), 1, 4), text);
        REFUSED(banded(weighted(plain(om), &setW, 1, 0, &pw, 1), M, 4, om.quality.data()), text);
        std::snprintf(text, sizeof text, "lag_bounds of group 1, %s", tail);
        REFUSED(grouped(weighted(plain(o), nullptr, 0, 0, &pg, 1), 2), text);
        std::snprintf(text, sizeof text, "lag_bounds of group -1, %s", tail);
        REFUSED(grouped(weighted(plain(o), nullptr, 0, 0, &sh, 0), 2, 0, o.quality.data()), text);
    }
    // with a custom list of one pair the rows are one pair long
    const std::vector<int32_t> one_pair = {0, 2};
    std::vector<int32_t> lb1 = bounds_of(W * 1);
    lb1[2 * 3] = 9; lb1[2 * 3 + 1] = 8;
    REFUSED(bounded(plain(o, W, one_pair.data(), 1), &lb1, 1), "lag_bounds of window 3, pair 0: [9, 8] is not an interval inside [-15, 15]");
    // refine
    for (int u : {1, 3, -2, 32}) {
        char text[128];
        std::snprintf(text, sizeof text, "refine = %d: the fine grid is 1 / U samples with U one of 0 (none), 2, 4, 8, 16", u);
        REFUSED(grouped(plain(o), 1, u), text);
        REFUSED(banded(weighted(plain(om), &set, 0, 0), M, u), text);
        REFUSED(banded(weighted(plain(o), &band1, 0, 0), 1, u), text);
    }
    // quality over another output, the array named: the same address, quality's first float on the array's last, the array's
    // first on quality's last (both inside one block, so no other array is near)
    for (int k = 0; k < 3; ++k) {
        static const char* name[3] = {"lag_int", "lag_frac", "peak"};
        auto with_out = [k](RequestArgs a, float* p) {
            if (k == 0) a.lag_int = reinterpret_cast<int32_t*>(p);
            if (k == 1) a.lag_frac = p;
            if (k == 2) a.peak = p;
            return a;
        };
        char text[128];
        for (int shape = 0; shape < 3; ++shape) {   // [W][P], the [G][P] of an integrated call, [W][M][P]
            const size_t slots = shape == 0 ? W * P : shape == 1 ? 2 * P : W * M * P;
            std::snprintf(text, sizeof text, "quality overlaps %s: the %zu x 4 floats of quality need a buffer of their own", name[k], slots);
            std::vector<float> block(5 * slots - 1);
            auto call = [&](float* out, float* quality, int refine) {
                if (shape == 2) return banded(weighted(with_out(plain(om), out), &setW, 1, RMX_WEIGHT_PHAT), M, refine, quality);
                return grouped(with_out(plain(o), out), shape == 1 ? 2 : 1, refine, quality);
            };
            REFUSED(call(block.data(), block.data(), 0), text);
            REFUSED(call(block.data(), block.data() + slots - 1, 8), text);
            REFUSED(call(block.data() + 4 * slots - 1, block.data(), 0), text);
            // quality ON the array also runs over the three arrays' worth of memory behind it: whichever output the
            // allocator placed there, the array that holds quality's first float is the one named
            if (shape != 2) {
                std::vector<float> row(4 * slots);
                RequestArgs a = grouped(plain(o), shape == 1 ? 2 : 1, 0, row.data());
                float* near[2] = {row.data() + slots, row.data() + 2 * slots};
                if (k == 0) { a.lag_int = reinterpret_cast<int32_t*>(row.data()); a.lag_frac = near[0]; a.peak = near[1]; }
                if (k == 1) { a.lag_frac = row.data(); a.lag_int = reinterpret_cast<int32_t*>(near[0]); a.peak = near[1]; }
                if (k == 2) { a.peak = row.data(); a.lag_int = reinterpret_cast<int32_t*>(near[0]); a.lag_frac = near[1]; }
                REFUSED(a, text);
            }
            std::vector<float> apart(5 * slots);
            (void)ACCEPTED(call(apart.data(), apart.data() + slots, 4));      // directly behind it
            (void)ACCEPTED(call(apart.data() + 4 * slots, apart.data(), 4));  // directly in front of it
        }
    }
}

// ---- 1b. a device pointer aligned to less than its element: refused, the array named; a host pointer is not looked at ----------
static void test_alignment() {
    Outs o((size_t)W * P + 1);
    std::vector<float> iq_block(8);
    char* const iq8 = reinterpret_cast<char*>(iq_block.data());            // a heap block: aligned to 8 or better
    const unsigned in_dev = RMX_IN_DEVICE, out_dev = RMX_OUT_DEVICE, both = in_dev | out_dev;
    auto call = [&](unsigned flags, const void* iq) {
        RequestArgs a = plain(o);
        a.flags = flags;
        a.iq = iq;
        return a;
    };
    // complex64 input: 8 bytes, one sample
    (void)ACCEPTED(call(both, iq8));
    (void)ACCEPTED(call(both, iq8 + 8));
    REFUSED(call(in_dev, iq8 + 4), "iq is a device pointer 4 bytes past a multiple of 8: complex64 input must be aligned to 8 bytes (one sample)");
    REFUSED(call(both, iq8 + 1), "iq is a device pointer 1 bytes past a multiple of 8: complex64 input must be aligned to 8 bytes (one sample)");
    (void)ACCEPTED(call(out_dev, iq8 + 4));                                  // a host pointer goes through the library's copy
    (void)ACCEPTED(call(0, iq8 + 1));
    // uint8 input: 2 bytes, one I,Q pair; an odd address is refused
    (void)ACCEPTED(call(both | RMX_IN_U8, iq8 + 2));
    (void)ACCEPTED(call(in_dev | RMX_IN_U8, iq8 + 6));
    REFUSED(call(both | RMX_IN_U8, iq8 + 1), "iq is a device pointer 1 bytes past a multiple of 2: uint8 input must be aligned to 2 bytes (one I,Q pair)");
    REFUSED(call(in_dev | RMX_IN_U8, iq8 + 7), "iq is a device pointer 1 bytes past a multiple of 2: uint8 input must be aligned to 2 bytes (one I,Q pair)");
    (void)ACCEPTED(call(out_dev | RMX_IN_U8, iq8 + 1));
    // the outputs: 4 bytes each, the first misaligned one named; every 4-byte offset is accepted
    for (int k = 0; k < 4; ++k) {
        static const char* name[4] = {"lag_int", "lag_frac", "peak", "quality"};
        for (int past = 0; past < 4; ++past) {
            RequestArgs a = grouped(call(both, iq8), 1, 0, o.quality.data());
            if (k == 0) a.lag_int = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(o.lag_int.data()) + past);
            if (k == 1) a.lag_frac = reinterpret_cast<float*>(reinterpret_cast<char*>(o.lag_frac.data()) + past);
            if (k == 2) a.peak = reinterpret_cast<float*>(reinterpret_cast<char*>(o.peak.data()) + past);
            if (k == 3) a.quality = reinterpret_cast<float*>(reinterpret_cast<char*>(o.quality.data()) + past);
            if (past == 0) {
                (void)ACCEPTED(a);
                continue;
            }
            char text[160];
            std::snprintf(text, sizeof text, "%s is a device pointer %d bytes past a multiple of 4: an output must be aligned to 4 bytes (one element)",
                          name[k], past);
            REFUSED(a, text);
            a.flags = in_dev;                                                // host outputs: not looked at
            (void)ACCEPTED(a);
        }
    }
    {   // lag_int one ELEMENT further (4 mod 16, 8 mod 16, ...): what a slice of a larger buffer gives
        RequestArgs a = call(both, iq8);
        a.lag_int = o.lag_int.data() + 1;
        (void)ACCEPTED(a);
    }
    // the order: behind a NULL buffer, in front of n_bands and everything after it; iq in front of the outputs
    const std::vector<double> set = bands_of(M);
    Outs om((size_t)W * M * P);
    {
        RequestArgs a = banded(weighted(plain(om), &set, 0, 7), 0, 3);
        a.flags = both;
        a.iq = iq8 + 4;
        a.peak = reinterpret_cast<float*>(reinterpret_cast<char*>(om.peak.data()) + 2);
        REFUSED(a, "iq is a device pointer 4 bytes past a multiple of 8: complex64 input must be aligned to 8 bytes (one sample)");
        a.iq = iq8;
        REFUSED(a, "peak is a device pointer 2 bytes past a multiple of 4: an output must be aligned to 4 bytes (one element)");
        a.lag_frac = nullptr;
        REFUSED(a, kNull);
    }
    // the Doppler search calls the same routine with its five outputs, a NULL dop_frac skipped
    {
        std::vector<int32_t> dop_idx((size_t)W * P);
        std::string err;
        const OutArray ok[5] = {{"dop_idx", dop_idx.data()}, {"dop_frac", nullptr}, {"lag_int", o.lag_int.data()}, {"lag_frac", o.lag_frac.data()},
                                {"peak", o.peak.data()}};
        CHECK(check_alignment(both, iq8, ok, 5, &err) == RMX_OK);
        const OutArray bad[5] = {{"dop_idx", reinterpret_cast<char*>(dop_idx.data()) + 3}, {"dop_frac", nullptr}, {"lag_int", o.lag_int.data()},
                                 {"lag_frac", o.lag_frac.data()}, {"peak", o.peak.data()}};
        CHECK(check_alignment(both, iq8, bad, 5, &err) == RMX_E_INVAL &&
              err == "dop_idx is a device pointer 3 bytes past a multiple of 4: an output must be aligned to 4 bytes (one element)");
        CHECK(check_alignment(in_dev, iq8, bad, 5, &err) == RMX_OK);
    }
}

// ---- 2. the order: a call bad in two adjacent classes is refused for the earlier one -------------------------------------------
static void test_refusal_order() {
    Outs o((size_t)W * P), om((size_t)W * M * P);
    const std::vector<double> set = bands_of(M), band1 = bands_of(1);
    std::vector<double> bad_set = set, bad_band = band1;
    bad_set[2] = 0.3; bad_set[3] = -0.2;
    bad_band[0] = 0.3; bad_band[1] = -0.2;
    std::vector<int32_t> bad_lb = bounds_of(P), bad_lbw = bounds_of(W * P);
    bad_lb[2] = 7; bad_lb[3] = 6;
    bad_lbw[2] = 7; bad_lbw[3] = 6;
    float* over = o.peak.data();
    float* over_m = om.peak.data();
    const char* band_text = "band of window 0 (one band shared by every window): [0.3, -0.2] is not an interval inside [-0.5, 0.5] cycles per sample";
    const char* set_text = "band 1 of window 0 (one band set shared by every window): [0.3, -0.2] is not an interval inside [-0.5, 0.5] cycles per sample";
    const char* lb_text = "lag_bounds of window -1, pair 1: [7, 6] is not an interval inside [-15, 15]";
    // the grouped checks before a NULL buffer; integrate before the group count
    {
        RequestArgs a = grouped(plain(o), 3);
        a.iq = nullptr;
        REFUSED(a, "n_windows = 4 is not a positive multiple of integrate = 3");
        a.integrate = 0;
        REFUSED(a, "integrate = 0: at least one window per group");
        REFUSED(grouped(plain(o, 5), 0), "integrate = 0: at least one window per group");
        // the pair count that sizes an integrated call's full intervals is looked at with them
        const std::vector<int32_t> two = {0, 1, 1, 2};
        RequestArgs b = grouped(plain(o, W, two.data(), -1), 2);
        b.iq = nullptr;
        REFUSED(b, "n_pairs -1 < 0");
        b.integrate = 1;
        REFUSED(b, kNull);
    }
    // a NULL buffer before n_bands (and lag_bounds == NULL of the bounded entry before everything)
    REFUSED(banded(weighted(plain(om), nullptr, 0, 7), 0, 3, over_m), kNull);
    REFUSED(bounded(plain(o, W + 1, nullptr, 2), nullptr, 0), kNull);
    {
        RequestArgs a = weighted(plain(o), &bad_band, 0, 7, &bad_lb, 0);
        a.peak = nullptr;
        REFUSED(a, kNull);                                                   // NULL before the weighting
    }
    // n_bands before the weighting
    REFUSED(banded(weighted(plain(om), &bad_set, 0, 7), 0, 3, over_m), "n_bands 0 not in 1..64");
    // the weighting before n_windows before the band
    REFUSED(banded(weighted(plain(om, W + 1), &bad_set, 0, 7, &bad_lb, 0), M, 3, over_m), kWeighting);
    REFUSED(weighted(plain(o, W + 1), &bad_band, 0, 7, &bad_lb, 0), kWeighting);
    REFUSED(grouped(weighted(plain(o), &bad_band, 0, 7, &bad_lb, 0), 2, 3, over), kWeighting);
    REFUSED(weighted(plain(o, W + 1), &bad_band, 0, 0), "n_windows 5 not in 0..max_windows=4");
    REFUSED(banded(weighted(plain(om, -1), &bad_set, 0, 0), M), "n_windows -1 not in 0..max_windows=4");
    // the band before the batch shape
    REFUSED(weighted(plain(o, W, nullptr, 2), &bad_band, 0, 0, &bad_lb, 0), band_text);
    REFUSED(banded(weighted(plain(om, W, nullptr, 2), &bad_set, 0, RMX_WEIGHT_PHAT, &bad_lb, 0), M, 3, over_m), set_text);
    // the batch shape before the bounds
    REFUSED(bounded(plain(o, W, nullptr, 2), &bad_lb, 0), "pairs == NULL needs n_pairs == 0 or 3, got 2");
    REFUSED(bounded(plain(o, W + 1), &bad_lb, 0), "n_windows 5 not in 0..max_windows=4");
    REFUSED(banded(weighted(plain(om, W, nullptr, 2), &set, 0, 0, &bad_lb, 0), M, 3, over_m), "pairs == NULL needs n_pairs == 0 or 3, got 2");
    REFUSED(grouped(weighted(plain(o, W, nullptr, 2), nullptr, 0, RMX_WEIGHT_PHAT, &bad_lb, 0), 2, 3, over),
            "pairs == NULL needs n_pairs == 0 or 3, got 2");
    // the bounds before refine
    REFUSED(grouped(weighted(plain(o), nullptr, 0, RMX_WEIGHT_PHAT, &bad_lb, 0), 1, 3, over), lb_text);
    REFUSED(grouped(weighted(plain(o), nullptr, 0, RMX_WEIGHT_PHAT, &bad_lb, 0), 2, 3, over),
            "lag_bounds of group -1, pair 1: [7, 6] is not an interval inside [-15, 15]");
    REFUSED(banded(weighted(plain(om), &set, 0, 0, &bad_lbw, 1), M, 3, over_m),
            "lag_bounds of window 0, pair 1: [7, 6] is not an interval inside [-15, 15]");
    // refine before the overlap
    REFUSED(grouped(plain(o), 2, 3, over), kRefine);
    REFUSED(banded(weighted(plain(om), &set, 0, 0), M, 3, over_m), kRefine);
    REFUSED(banded(weighted(plain(o), &band1, 0, 0), 1, 3, over), kRefine);
}

// ---- the tail of rmx_caf_batch_request: weighted, then bounded, then dop_frac --------------------------------------------------
static int caf(const RequestArgs& a, const std::vector<int32_t>& dop_idx, const float* dop_frac, Request* r, std::string* err) {
    return check_caf_request(a, dop_idx.data(), dop_frac, r, err);
}
static void test_caf_tail() {
    Outs o((size_t)W * P);
    std::vector<int32_t> dop_idx((size_t)W * P);
    std::vector<float> dop_frac((size_t)W * P);
    const std::vector<double> band1 = bands_of(1);
    std::vector<double> bad_band = band1, thin = band1, nanW = bands_of(W);
    bad_band[0] = 0.3; bad_band[1] = -0.2;
    thin[0] = 0.1 / N; thin[1] = 0.2 / N;
    nanW[2] = NaN;
    const std::vector<int32_t> lb = bounds_of(P);
    std::vector<int32_t> bad_lb = lb, few = bounds_of(W * P);
    bad_lb[2] = 4; bad_lb[3] = 3;
    few[2 * P] = -N; few[2 * P + 1] = 0;
    Request r;
    std::string err;
    auto refused_caf = [&](const RequestArgs& a, const float* df, const char* text) {
        return caf(a, dop_idx, df, &r, &err) == RMX_E_INVAL && err == text;
    };
    float* over = o.peak.data();
    CHECK(refused_caf(weighted(plain(o), nullptr, 0, 7), dop_frac.data(), kWeighting));
    CHECK(refused_caf(weighted(plain(o), &bad_band, 0, 7, &bad_lb, 0), over, kWeighting));           // the weighting, then the band,
    CHECK(refused_caf(weighted(plain(o), &bad_band, 0, 0, &bad_lb, 0), over,
                      "band of window 0 (one band shared by every window): [0.3, -0.2] is not an interval inside [-0.5, 0.5] cycles per sample"));
    CHECK(refused_caf(weighted(plain(o), &thin, 0, 0), nullptr,
                      "band of window 0 (one band shared by every window): [0.00625, 0.0125] keeps no bin of the 32-point transform"));
    CHECK(refused_caf(weighted(plain(o), &nanW, 1, 0), nullptr,
                      "band of window 1: [nan, 0.25] is not an interval inside [-0.5, 0.5] cycles per sample"));
    CHECK(refused_caf(weighted(plain(o), nullptr, 0, RMX_WEIGHT_PHAT, &bad_lb, 0), over,              // then the bounds,
                      "lag_bounds of window -1, pair 1: [4, 3] is not an interval inside [-15, 15]"));
    CHECK(refused_caf(weighted(plain(o), &band1, 0, 0, &few, 1), over,
                      "lag_bounds of window 1, pair 0: [-16, 0] is not an interval inside [-15, 15]"));
    // then dop_frac over another output, whichever it lies over (both inside one block, so no other array is near)
    for (int k = 0; k < 4; ++k) {
        static const char* name[4] = {"dop_idx", "lag_int", "lag_frac", "peak"};
        const std::string text = std::string("dop_frac overlaps ") + name[k] + ": its 12 floats need a buffer of their own";
        const size_t slots = (size_t)W * P;
        std::vector<float> block(2 * slots - 1), apart(2 * slots);
        auto call = [&](float* out, const float* df, const int32_t** di) {
            RequestArgs a = weighted(plain(o), nullptr, 0, RMX_WEIGHT_PHAT, &lb, 0);
            *di = k == 0 ? reinterpret_cast<const int32_t*>(out) : dop_idx.data();
            if (k == 1) a.lag_int = reinterpret_cast<int32_t*>(out);
            if (k == 2) a.lag_frac = out;
            if (k == 3) a.peak = out;
            (void)df;
            return a;
        };
        const int32_t* di = nullptr;
        RequestArgs a = call(block.data(), block.data(), &di);
        CHECK(check_caf_request(a, di, block.data(), &r, &err) == RMX_E_INVAL && err == text);
        CHECK(check_caf_request(a, di, block.data() + slots - 1, &r, &err) == RMX_E_INVAL && err == text);
        a = call(block.data() + slots - 1, block.data(), &di);
        CHECK(check_caf_request(a, di, block.data(), &r, &err) == RMX_E_INVAL && err == text);
        a = call(apart.data(), apart.data() + slots, &di);
        CHECK(check_caf_request(a, di, apart.data() + slots, &r, &err) == RMX_OK);
    }
    // accepted: the plain request, and the staged form of a full one
    CHECK(caf(plain(o), dop_idx, nullptr, &r, &err) == RMX_OK && !r.weighted && !r.bounded && r.bins.empty() && r.own_bounds.empty());
    const std::vector<double> bandW = bands_of(W, -0.5, 0.25);
    CHECK(caf(weighted(plain(o), &bandW, 1, RMX_WEIGHT_PHAT, &few, 0), dop_idx, dop_frac.data(), &r, &err) == RMX_OK);
    CHECK(r.weighted && r.phat && r.band_per_window && r.n_bands == 1 && r.bins.size() == 2 * (size_t)W && r.bins[0] == -N && r.bins[1] == 8);
    CHECK(r.bounded && !r.bounds_per_window && r.bound_rows == P && r.bounds == few.data() && r.n_pairs == P);
    // the full band without weighting and full intervals: the plain search
    const std::vector<double> full = bands_of(1, -0.5, 0.5);
    const std::vector<int32_t> full_lb = bounds_of(P, -(N - 1), N - 1);
    CHECK(caf(weighted(plain(o), &full, 0, 0, &full_lb, 0), dop_idx, dop_frac.data(), &r, &err) == RMX_OK && !r.weighted && !r.bounded);
}

// ---- the head of the Doppler entries, in front of that tail: NULL buffer, alignment of the five arrays, n_dopplers, the group
// count (integrate != 1 only), the batch shape, the empty batch, the pair list ------------------------------------------------------
// The WHOLE check, as caf_request in rmx_hip.hip calls it: the arguments as an entry fills them (the grid and the search's own
// two outputs in RequestArgs)
static const double kGrid[3] = {-1e-4, 0.0, 1e-4};
static int check_caf(RequestArgs a, const int32_t* dop_idx, const float* dop_frac, Request* r, std::string* err) {
    if (!a.doppler_cps && a.n_dopplers == 0) {
        a.doppler_cps = kGrid;
        a.n_dopplers = 3;
    }
    a.dop_idx = const_cast<int32_t*>(dop_idx);
    a.dop_frac = const_cast<float*>(dop_frac);
    return check_caf_request(a, r, err);
}
static void test_caf_head() {
    Outs o((size_t)W * P);
    std::vector<int32_t> dop_idx((size_t)W * P);
    std::vector<float> dop_frac((size_t)W * P);
    const std::vector<double> band1 = bands_of(1);
    std::vector<double> bad_band = band1;
    bad_band[0] = 0.3; bad_band[1] = -0.2;
    std::vector<int32_t> bad_lb = bounds_of(P);
    bad_lb[2] = 4; bad_lb[3] = 3;
    const std::vector<int32_t> bad_pairs = {0, 1, 0, 3, 1, 2}, rev = {1, 2, 0, 2, 0, 1};
    Request r;
    std::string err;
    auto refused_caf = [&](const RequestArgs& a, const int32_t* di, const float* df, const char* text) {
        const int rc = check_caf(a, di, df, &r, &err);
        if (rc != RMX_E_INVAL || err != text) std::fprintf(stderr, "rc %d, text \"%s\"\n  wanted \"%s\"\n", rc, err.c_str(), text);
        return rc == RMX_E_INVAL && err == text;
    };
    const int32_t* di = dop_idx.data();
    const float* df = dop_frac.data();
    const char* past2 = reinterpret_cast<const char*>(df) + 2;
    // everything at once that the tail refuses: a bad weighting, a bad band, bad bounds, refine = 3, quality over peak
    const RequestArgs bad_tail = grouped(weighted(plain(o), &bad_band, 0, 7, &bad_lb, 0), 1, 3, o.peak.data());
    // a NULL buffer: each of the six the plain search takes (dop_frac and quality may be NULL), in front of everything else
    for (int k = 0; k < 6; ++k) {
        RequestArgs a = bad_tail;
        a.n_dopplers = k == 5 ? 3 : 9999;   // (k == 5: doppler_cps stays NULL)
        a.doppler_cps = k == 5 ? nullptr : kGrid;
        a.flags = RMX_OUT_DEVICE;
        if (k == 0) a.iq = nullptr;
        if (k == 2) a.lag_int = nullptr;
        if (k == 3) a.lag_frac = nullptr;
        if (k == 4) a.peak = nullptr;
        CHECK(refused_caf(a, k == 1 ? nullptr : di, reinterpret_cast<const float*>(past2), kNull));
    }
    // a misaligned device pointer: in the order dop_idx, dop_frac, lag_int, lag_frac, peak, in front of n_dopplers
    {
        RequestArgs a = bad_tail;
        a.doppler_cps = kGrid;
        a.n_dopplers = 0;
        a.flags = RMX_OUT_DEVICE;
        a.lag_int = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(o.lag_int.data()) + 1);
        CHECK(refused_caf(a, di, reinterpret_cast<const float*>(past2),
                          "dop_frac is a device pointer 2 bytes past a multiple of 4: an output must be aligned to 4 bytes (one element)"));
        CHECK(refused_caf(a, di, df, "lag_int is a device pointer 1 bytes past a multiple of 4: an output must be aligned to 4 bytes (one element)"));
        CHECK(refused_caf(a, reinterpret_cast<const int32_t*>(past2), reinterpret_cast<const float*>(past2),
                          "dop_idx is a device pointer 2 bytes past a multiple of 4: an output must be aligned to 4 bytes (one element)"));
        a.flags = RMX_IN_DEVICE;   // host outputs need nothing; a device iq does
        a.iq = reinterpret_cast<const char*>(g_iq.data()) + 4;
        CHECK(refused_caf(a, di, df, "iq is a device pointer 4 bytes past a multiple of 8: complex64 input must be aligned to 8 bytes (one sample)"));
        a.flags = 0;
        CHECK(refused_caf(a, di, reinterpret_cast<const float*>(past2), "n_dopplers 0 not in 1..4096"));
    }
    // n_dopplers in front of the group count, the batch shape, the pair list and the whole tail
    for (int d : {0, -1, 4097}) {
        RequestArgs a = grouped(weighted(plain(o, W + 1, bad_pairs.data(), P), &bad_band, 0, 7, &bad_lb, 0), 3, 3, o.peak.data());
        a.doppler_cps = kGrid;
        a.n_dopplers = d;
        char want[48];
        std::snprintf(want, sizeof want, "n_dopplers %d not in 1..4096", d);
        CHECK(refused_caf(a, di, o.peak.data(), want));
    }
    // the group count (integrate != 1 only) in front of the batch shape; one window per group looks at the batch shape alone
    CHECK(refused_caf(grouped(weighted(plain(o, W + 1, bad_pairs.data(), P), &bad_band, 0, 7), 3), di, df,
                      "n_windows = 5 is not a positive multiple of integrate = 3"));
    CHECK(refused_caf(grouped(plain(o, W, bad_pairs.data(), P), 0), di, df, "integrate = 0: at least one window per group"));
    CHECK(refused_caf(grouped(plain(o, 0), 2), di, df, "n_windows = 0 is not a positive multiple of integrate = 2"));
    CHECK(refused_caf(grouped(weighted(plain(o, W + 1, bad_pairs.data(), P), &bad_band, 0, 7), 1), di, df, "n_windows 5 not in 0..max_windows=4"));
    // the batch shape in front of the pair list and the tail
    CHECK(refused_caf(weighted(plain(o, W, nullptr, 2), &bad_band, 0, 7, &bad_lb, 0), di, df, "pairs == NULL needs n_pairs == 0 or 3, got 2"));
    CHECK(refused_caf(weighted(plain(o, W, bad_pairs.data(), -1), &bad_band, 0, 7), di, df, "n_pairs -1 < 0"));
    // the empty batch is OK before its pairs, its bands and its refine are looked at (one window per group only)
    CHECK(check_caf(grouped(weighted(plain(o, 0, bad_pairs.data(), P), &bad_band, 0, 7, &bad_lb, 0), 1, 3, o.peak.data()), di, o.peak.data(), &r, &err) == RMX_OK && r.empty);
    CHECK(check_caf(weighted(plain(o, W, bad_pairs.data(), 0), &bad_band, 0, 7), di, df, &r, &err) == RMX_OK && r.empty && r.n_pairs == 0);
    // the pair list in front of the weighting, the band, the bounds and everything behind them
    const char* pair_text = "pair 1 = (0,3) out of range for 3 buoys";
    CHECK(refused_caf(weighted(plain(o, W, bad_pairs.data(), P), &bad_band, 0, 7, &bad_lb, 0), di, o.peak.data(), pair_text));
    CHECK(refused_caf(weighted(plain(o, W, bad_pairs.data(), P), &bad_band, 0, 0), di, df, pair_text));
    CHECK(refused_caf(grouped(plain(o, W, bad_pairs.data(), P), 2, 3, o.peak.data()), di, df, pair_text));
    const std::vector<int32_t> neg = {0, 1, -1, 2};
    CHECK(refused_caf(plain(o, W, neg.data(), 2), di, df, "pair 1 = (-1,2) out of range for 3 buoys"));
    // ... and a good list hands the tail its first refusal
    CHECK(refused_caf(weighted(plain(o, W, rev.data(), P), &bad_band, 0, 7, &bad_lb, 0), di, o.peak.data(), kWeighting));
    // accepted: a custom list, its length resolved; the default one by its count
    CHECK(check_caf(plain(o, W, rev.data(), P), di, df, &r, &err) == RMX_OK && !r.empty && r.n_pairs == P);
    CHECK(check_caf(plain(o, W, rev.data(), 2), di, df, &r, &err) == RMX_OK && r.n_pairs == 2);
    CHECK(check_caf(plain(o, W, nullptr, 0), di, df, &r, &err) == RMX_OK && r.n_pairs == P);
    for (int d : {1, 4096}) {
        RequestArgs a = plain(o);
        a.doppler_cps = kGrid;   // (only counted by the check, never read)
        a.n_dopplers = d;
        CHECK(check_caf(a, di, nullptr, &r, &err) == RMX_OK);
    }
}

// ---- 3. the empty batches and the identities --------------------------------------------------------------------------------
static void test_empty_and_identities() {
    Outs o((size_t)W * P), om((size_t)W * M * P);
    const std::vector<double> band1 = bands_of(1), set = bands_of(M), full = bands_of(1, -0.5, 0.5);
    const std::vector<int32_t> one_pair = {0, 2};
    // arrays of no rows: not NULL, and not one element long
    const std::unique_ptr<double[]> no_bands(new double[0]);
    const std::unique_ptr<int32_t[]> no_pairs(new int32_t[0]), no_lb(new int32_t[0]);
    // a weighted or banded call without windows is OK before its pairs are looked at; its per-window arrays have no rows
    Request r = ACCEPTED(weighted(plain(o, 0, nullptr, 2), &band1, 0, 0));
    CHECK(r.empty);
    r = ACCEPTED(weighted(plain(o, 0, nullptr, 2), nullptr, 0, RMX_WEIGHT_PHAT));
    CHECK(r.empty);
    RequestArgs a = weighted(plain(o, 0, nullptr, 2), nullptr, 1, RMX_WEIGHT_PHAT);
    a.band_cps = no_bands.get();
    r = ACCEPTED(a);
    CHECK(r.empty);
    r = ACCEPTED(banded(weighted(plain(om, 0, nullptr, 2), &set, 0, 0), M, 3, nullptr));              // (refine is not looked at either)
    CHECK(r.empty);
    a = banded(weighted(plain(om, 0, one_pair.data(), -1), nullptr, 1, 0), M);
    a.band_cps = no_bands.get();
    r = ACCEPTED(a);
    CHECK(r.empty);
    r = ACCEPTED(banded(weighted(plain(o, 0, nullptr, 2), &band1, 0, 0), 1));                         // n_bands == 1 with a band: weighted
    CHECK(r.empty);
    // ... but the plain call looks at them: the full band without weighting is the plain call, through either entry
    REFUSED(weighted(plain(o, 0, nullptr, 2), &full, 0, 0), "pairs == NULL needs n_pairs == 0 or 3, got 2");
    REFUSED(banded(weighted(plain(o, 0, nullptr, 2), &full, 0, 0), 1), "pairs == NULL needs n_pairs == 0 or 3, got 2");
    REFUSED(plain(o, 0, nullptr, 2), "pairs == NULL needs n_pairs == 0 or 3, got 2");
    // otherwise no windows or no pairs is OK before the bounds (of which there are then no rows) and before refine
    const std::vector<int32_t> lbP = bounds_of(P, 5, 4);
    r = ACCEPTED(plain(o, 0));
    CHECK(r.empty);
    r = ACCEPTED(bounded(plain(o, 0), &lbP, 0));
    CHECK(r.empty);
    a = bounded(plain(o, W, no_pairs.get(), 0), &lbP, 1);
    a.lag_bounds = no_lb.get();
    r = ACCEPTED(a);
    CHECK(r.empty && r.n_pairs == 0);
    a = grouped(weighted(plain(o, W, no_pairs.get(), 0), &band1, 0, 0, &lbP, 0), 2, 3);
    a.lag_bounds = no_lb.get();
    r = ACCEPTED(a);
    CHECK(r.empty);
    a = banded(weighted(plain(om, W, no_pairs.get(), 0), &set, 0, 0, &lbP, 1), M, 3);
    a.lag_bounds = no_lb.get();
    r = ACCEPTED(a);
    CHECK(r.empty);
    // the plain call: nothing allocated, nothing to stage
    r = ACCEPTED(plain(o));
    CHECK(!r.empty && r.n_pairs == P && !r.weighted && !r.bounded && r.n_bands == 1 && r.integ == 1 && r.refine == 0);
    CHECK(r.bins.capacity() == 0 && r.own_bounds.capacity() == 0);
    r = ACCEPTED(plain(o, W, nullptr, 0));
    CHECK(r.n_pairs == P);
    r = ACCEPTED(plain(o, 2, one_pair.data(), 1));
    CHECK(r.n_pairs == 1 && !r.empty);
    // a full band (or none) without weighting is not weighted; with PHAT it is
    r = ACCEPTED(weighted(plain(o), &full, 0, 0));
    CHECK(!r.weighted);
    r = ACCEPTED(weighted(plain(o), nullptr, 0, RMX_WEIGHT_PHAT));
    CHECK(r.weighted && r.phat && r.bins == (std::vector<int32_t>{-N, N - 1}) && !r.band_per_window);
    // [-0.5, 0.5 - 1/L] keeps every bin too
    const std::vector<double> all_bins = bands_of(W, -0.5, 0.5 - 1.0 / (2 * N));
    r = ACCEPTED(weighted(plain(o), &all_bins, 1, 0));
    CHECK(!r.weighted);
    // bounded is false only when every interval is full and integrate == 1
    std::vector<int32_t> full_lb = bounds_of(W * P, -(N - 1), N - 1);
    r = ACCEPTED(bounded(plain(o), &full_lb, 1));
    CHECK(!r.bounded);
    r = ACCEPTED(grouped(weighted(plain(o), nullptr, 0, 0, &full_lb, 0), 1));
    CHECK(!r.bounded);
    r = ACCEPTED(grouped(weighted(plain(o), nullptr, 0, 0, &full_lb, 0), 2));
    CHECK(r.bounded && r.integ == 2);
    full_lb[2 * (W * P - 1)] = -(N - 2);
    r = ACCEPTED(bounded(plain(o), &full_lb, 1));
    CHECK(r.bounded && r.bounds == full_lb.data() && r.bound_rows == W * P && r.bounds_per_window && r.own_bounds.empty());
    // n_bands == 1 is exactly the weighted request: no [full band | prefix, no band set, and a full band is not weighted
    const std::vector<double> bandW = bands_of(W, -0.125, 0.25);
    const Request rb = ACCEPTED(banded(weighted(plain(o), &bandW, 1, RMX_WEIGHT_PHAT, &full_lb, 1), 1, 4, o.quality.data()));
    const Request rw = ACCEPTED(grouped(weighted(plain(o), &bandW, 1, RMX_WEIGHT_PHAT, &full_lb, 1), 1, 4, o.quality.data()));
    CHECK(rb.n_bands == 1 && rb.bins.size() == 2 * (size_t)W && rb.bins == rw.bins && rb.weighted && rw.weighted && rb.phat && rw.phat);
    CHECK(rb.band_per_window && rw.band_per_window && rb.bounded && rw.bounded && rb.bounds == rw.bounds && rb.bound_rows == rw.bound_rows);
    CHECK(rb.bounds_per_window == rw.bounds_per_window && rb.refine == 4 && rw.refine == 4 && rb.integ == 1 && rb.own_bounds.empty());
    r = ACCEPTED(banded(weighted(plain(o), &full, 0, 0), 1));
    CHECK(!r.weighted && r.n_bands == 1);
    // refine == 0 && quality == NULL through _bands_quality is the _bands request (the same arguments: one function)
    r = ACCEPTED(banded(weighted(plain(om), &set, 0, 0), M, 0, nullptr));
    CHECK(r.n_bands == M && r.refine == 0 && r.weighted && !r.phat && !r.bounded);
    // quality in a buffer of its own, directly behind peak
    std::vector<float> block(5 * (size_t)W * P);
    a = grouped(plain(o), 1, 0, block.data() + W * P);
    a.peak = block.data();
    (void)ACCEPTED(a);
}

// ---- 4. the staged layouts, row by row ------------------------------------------------------------------------------------------
static void test_staged_layouts() {
    Outs o((size_t)W * P), om((size_t)W * M * P);
    // shared band and bounds.  L = 32: [-0.25, 0.26] keeps bins -8 .. 8; hi = 0.5 is bin 16, clamped to 15
    const std::vector<double> band = bands_of(1, -0.25, 0.26);
    std::vector<int32_t> lb = {-3, 3, -15, 15, 0, 0};
    Request r = ACCEPTED(weighted(plain(o), &band, 0, 0, &lb, 0));
    CHECK(r.weighted && !r.phat && !r.band_per_window && r.bins == (std::vector<int32_t>{-8, 8}));
    CHECK(r.bounded && r.bounds == lb.data() && r.bound_rows == P && !r.bounds_per_window && r.own_bounds.empty());
    // per-window band and bounds
    std::vector<double> bw(2 * (size_t)W);
    std::vector<int32_t> want;
    for (int w = 0; w < W; ++w) {
        bw[2 * w] = -0.5 + w / 32.0;
        bw[2 * w + 1] = 0.5 - w / 32.0;
        want.push_back(-N + w);
        want.push_back(w == 0 ? N - 1 : N - w);
    }
    std::vector<int32_t> lbw(2 * (size_t)W * P);
    for (int k = 0; k < W * P; ++k) {
        lbw[2 * k] = -k;
        lbw[2 * k + 1] = k;
    }
    r = ACCEPTED(weighted(plain(o), &bw, 1, RMX_WEIGHT_PHAT, &lbw, 1));
    CHECK(r.weighted && r.phat && r.band_per_window && r.bins == want);
    CHECK(r.bounded && r.bounds == lbw.data() && r.bound_rows == W * P && r.bounds_per_window && r.own_bounds.empty());
    // a custom list of two pairs: the rows are two pairs long
    const std::vector<int32_t> two = {0, 1, 1, 2};
    std::vector<int32_t> lb2(lbw.begin(), lbw.begin() + 2 * W * 2);
    r = ACCEPTED(bounded(plain(o, W, two.data(), 2), &lb2, 1));
    CHECK(r.n_pairs == 2 && r.bounded && r.bound_rows == W * 2 && r.bounds == lb2.data());
    // integrate = 2 without bounds: the full interval per pair, one row for every group
    r = ACCEPTED(grouped(plain(o), 2));
    CHECK(r.integ == 2 && r.bounded && !r.bounds_per_window && r.bound_rows == P && r.bounds == r.own_bounds.data());
    CHECK(r.own_bounds == (std::vector<int32_t>{-15, 15, -15, 15, -15, 15}) && !r.weighted && r.bins.empty());
    r = ACCEPTED(grouped(plain(o, W, two.data(), 2), 4, 8, o.quality.data()));
    CHECK(r.integ == 4 && r.refine == 8 && r.bounded && r.bound_rows == 2 && r.own_bounds == (std::vector<int32_t>{-15, 15, -15, 15}));
    // ... with per-group bounds: G = 2 rows of the caller's
    std::vector<int32_t> lbg(lbw.begin(), lbw.begin() + 2 * 2 * P);
    r = ACCEPTED(grouped(weighted(plain(o), nullptr, 0, 0, &lbg, 1), 2));
    CHECK(r.bounded && r.bounds == lbg.data() && r.bound_rows == 2 * P && r.bounds_per_window && r.own_bounds.empty());
    // M = 3, a shared band set: [full band | band set]
    std::vector<double> set = {-0.25, 0.26, 0.0, 0.5, -0.5, -0.375};
    r = ACCEPTED(banded(weighted(plain(om), &set, 0, 0), M));
    CHECK(r.n_bands == M && r.weighted && !r.band_per_window && r.bins == (std::vector<int32_t>{-16, 15, -8, 8, 0, 15, -16, -12}));
    // M = 3, per-window band sets and per-window bounds: each window's row of bounds M times, window-major
    std::vector<double> setw(2 * (size_t)W * M);
    want = {-16, 15};
    for (int k = 0; k < W * M; ++k) {
        setw[2 * k] = -k / 32.0;
        setw[2 * k + 1] = k / 32.0;
        want.push_back(-k);
        want.push_back(k);
    }
    r = ACCEPTED(banded(weighted(plain(om), &setw, 1, RMX_WEIGHT_PHAT, &lbw, 1), M, 4, om.quality.data()));
    CHECK(r.n_bands == M && r.weighted && r.phat && r.band_per_window && r.bins == want && r.refine == 4);
    CHECK(r.bounded && r.bounds_per_window && r.bound_rows == (long)W * M * P && r.bounds == r.own_bounds.data());
    CHECK(r.own_bounds.size() == 2 * (size_t)W * M * P);
    for (int w = 0; w < W; ++w)
        for (int m = 0; m < M; ++m)
            for (int q = 0; q < P; ++q) {
                const size_t k = ((size_t)(w * M + m) * P + q) * 2;
                CHECK(r.own_bounds[k] == -(w * P + q) && r.own_bounds[k + 1] == w * P + q);
            }
    // ... with shared bounds: the caller's one row, as it is
    r = ACCEPTED(banded(weighted(plain(om), &setw, 1, 0, &lb, 0), M));
    CHECK(r.bounded && !r.bounds_per_window && r.bound_rows == P && r.bounds == lb.data() && r.own_bounds.empty());
    // ... with per-window bounds that are all full: not bounded, nothing replicated
    const std::vector<int32_t> full_lb = bounds_of(W * P, -(N - 1), N - 1);
    r = ACCEPTED(banded(weighted(plain(om), &set, 0, 0, &full_lb, 1), M));
    CHECK(!r.bounded && r.own_bounds.empty());
}

int main() {
    test_refusal_texts();
    test_alignment();
    test_refusal_order();
    test_caf_head();
    test_caf_tail();
    test_empty_and_identities();
    test_staged_layouts();
    std::printf("all checks passed\n");
    return 0;
}
