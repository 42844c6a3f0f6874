// host::check_caf_request (radio-mapper_amd/csrc/host_request.hpp) with what rmx_caf_batch_quality adds -- refine, quality
// over one of the five other outputs, a misaligned device quality --, without a GPU: built with
// g++ -fsanitize=address,undefined by tests/test_caf_quality_request_sanitized.py.  The outputs are real arrays of exactly
// the stated sizes inside one slab, so a check that read past an array would be an AddressSanitizer report.
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

struct Outs {
    std::vector<float> slab;
    int32_t *dop, *lag;
    float *dfrac, *frac, *peak, *quality;
    explicit Outs(size_t slots) : slab(9 * slots, 0.0f) {
        float* p = slab.data();
        dop = reinterpret_cast<int32_t*>(p);
        dfrac = p + slots;
        lag = reinterpret_cast<int32_t*>(p + 2 * slots);
        frac = p + 3 * slots;
        peak = p + 4 * slots;
        quality = p + 5 * slots;   // 4 * slots floats: the slab ends with it
    }
};

static RequestArgs args(const Outs& o, int W, int P, int N) {
    RequestArgs a;
    a.n_buoys = 4;
    a.n_samples = N;
    a.max_windows = 64;
    a.iq = o.slab.data();   // (never read by the checks)
    a.n_windows = W;
    a.n_pairs = P;
    a.lag_int = o.lag;
    a.lag_frac = o.frac;
    a.peak = o.peak;
    a.quality = o.quality;
    a.refine = 8;
    return a;
}

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

int main() {
    const int W = 5, P = 6, N = 256;
    const size_t slots = (size_t)W * P;
    Outs o(slots);
    Request r;
    std::string err;

    // the request as asked: accepted, refine handed on, nothing else set
    RequestArgs a = args(o, W, P, N);
    CHECK(check_caf_request(a, o.dop, o.dfrac, &r, &err) == RMX_OK);
    CHECK(r.refine == 8 && r.n_pairs == P && !r.weighted && !r.bounded && r.integ == 1);
    for (int u : {0, 2, 4, 8, 16}) {
        a.refine = u;
        CHECK(check_caf_request(a, o.dop, o.dfrac, &r, &err) == RMX_OK && r.refine == u);
    }
    // neither: the request entry's own call
    a = args(o, W, P, N);
    a.refine = 0;
    a.quality = nullptr;
    CHECK(check_caf_request(a, o.dop, nullptr, &r, &err) == RMX_OK && r.refine == 0);

    // refine: every other value, with the value in the text
    for (int u : {-1, 1, 3, 5, 7, 9, 15, 17, 32}) {
        a = args(o, W, P, N);
        a.refine = u;
        err.clear();
        CHECK(check_caf_request(a, o.dop, o.dfrac, &r, &err) == RMX_E_INVAL);
        char want[32];
        std::snprintf(want, sizeof want, "refine = %d:", u);
        CHECK(has(err, want));
    }

    // quality over each of the five other outputs: on its first element, on its last, and running into it from in front
    struct { const char* name; const void* p; } others[5] = {
        {"dop_idx", o.dop}, {"dop_frac", o.dfrac}, {"lag_int", o.lag}, {"lag_frac", o.frac}, {"peak", o.peak}};
    for (const auto& other : others) {
        const float* base = static_cast<const float*>(other.p);
        for (const float* q : {base, base + slots - 1}) {
            a = args(o, W, P, N);
            a.quality = const_cast<float*>(q);
            err.clear();
            CHECK(check_caf_request(a, o.dop, o.dfrac, &r, &err) == RMX_E_INVAL);
            CHECK(has(err, "quality overlaps") && has(err, other.name) && has(err, "30 x 4 floats"));
        }
    }
    {   // a quality whose first byte lies in no array but whose tail covers dop_idx: a buffer of its own in front of the slab
        std::vector<float> big(4 * slots + slots, 0.0f);
        int32_t* dop2 = reinterpret_cast<int32_t*>(big.data() + 4 * slots - 1);   // the last float of quality is dop2[0]
        a = args(o, W, P, N);
        a.quality = big.data();
        err.clear();
        CHECK(check_caf_request(a, dop2, o.dfrac, &r, &err) == RMX_E_INVAL && has(err, "quality overlaps dop_idx"));
        // ... and one float earlier it does not
        a.quality = big.data();
        dop2 = reinterpret_cast<int32_t*>(big.data() + 4 * slots);
        CHECK(check_caf_request(a, dop2, o.dfrac, &r, &err) == RMX_OK);
    }
    // without dop_frac its (NULL) array is not looked at
    a = args(o, W, P, N);
    CHECK(check_caf_request(a, o.dop, nullptr, &r, &err) == RMX_OK);

    // the order: the weighted entry's, the bounded entry's, dop_frac's overlap, refine, quality's overlap, quality's alignment
    {
        a = args(o, W, P, N);
        a.weighting = 7;
        a.refine = 3;
        a.quality = o.peak;
        CHECK(check_caf_request(a, o.dop, o.peak, &r, &err) == RMX_E_INVAL && has(err, "unknown weighting 7"));
        a.weighting = RMX_WEIGHT_PHAT;
        const int32_t bad[2] = {5, 4};
        std::vector<int32_t> lb(2 * P, 0);
        std::memcpy(lb.data() + 2, bad, sizeof bad);
        a.lag_bounds = lb.data();
        CHECK(check_caf_request(a, o.dop, o.peak, &r, &err) == RMX_E_INVAL && has(err, "lag_bounds of window -1, pair 1"));
        a.lag_bounds = nullptr;
        CHECK(check_caf_request(a, o.dop, o.peak, &r, &err) == RMX_E_INVAL && has(err, "dop_frac overlaps peak"));
        CHECK(check_caf_request(a, o.dop, o.dfrac, &r, &err) == RMX_E_INVAL && has(err, "refine = 3:"));
        a.refine = 4;
        CHECK(check_caf_request(a, o.dop, o.dfrac, &r, &err) == RMX_E_INVAL && has(err, "quality overlaps peak"));
        // misaligned AND overlapping: the overlap is named first
        a.flags = RMX_OUT_DEVICE;
        a.quality = reinterpret_cast<float*>(reinterpret_cast<char*>(o.peak) + 2);
        CHECK(check_caf_request(a, o.dop, o.dfrac, &r, &err) == RMX_E_INVAL && has(err, "quality overlaps peak"));
    }
    // a misaligned quality is refused for a device pointer only
    for (unsigned past = 1; past < 4; ++past) {
        std::vector<char> own(4 * slots * sizeof(float) + 8);
        a = args(o, W, P, N);
        a.quality = reinterpret_cast<float*>(own.data() + past);
        a.flags = RMX_OUT_DEVICE;
        err.clear();
        CHECK(check_caf_request(a, o.dop, o.dfrac, &r, &err) == RMX_E_INVAL);
        char want[80];
        std::snprintf(want, sizeof want, "quality is a device pointer %u bytes past a multiple of 4", past);
        CHECK(has(err, want));
        a.flags = RMX_IN_DEVICE;   // host outputs pass through the library's own copies
        CHECK(check_caf_request(a, o.dop, o.dfrac, &r, &err) == RMX_OK);
    }

    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
