// The plan and the request of rmx_xcorr_batch_bands_integrated (radio-mapper_amd/csrc/host_plan.hpp, host_request.hpp)
// without a GPU: built with g++ -fsanitize=address,undefined by tests/test_bands_integ_plan_sanitized.py.  plan_route over
// n_bands x integrate x route: the chunk holds whole groups AND stays within plan_bands' caps, and the refusal fires
// exactly when no such chunk exists; the launch code's walk over rows group * n_bands + band writes every output slot
// once; check_request's bounds for a grouped AND banded call are indexed to their last row, so a layout one row short is
// an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
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

// the launch code's walk: chunks of p.chunk real windows; a chunk's work items are rows (group, band) x pairs, each
// walking the K real windows of its group, which must lie in the chunk
static void replay(const RoutePlan& p, int W, int K, int nb, int P) {
    std::vector<int> out((size_t)(W / K) * nb * P, 0);
    for (int w0 = 0; w0 < W; w0 += p.chunk) {
        const int wc = W - w0 < p.chunk ? W - w0 : p.chunk;
        CHECK(w0 % K == 0 && wc % K == 0);
        const long first_row = (long)(w0 / K) * nb, rows = (long)wc / K * nb;
        for (long r = 0; r < rows; ++r)
            for (int q = 0; q < P; ++q) {
                const long g = r / nb, m = r % nb;
                for (int kw = 0; kw < K; ++kw) {
                    const long wl = g * K + kw;                             // chunk-local real window
                    CHECK(wl >= 0 && wl < wc);
                    const long vslot = ((wl * nb) + m) * P + q;             // four-step: the product slot the banded rows wrote
                    CHECK(vslot < (long)wc * nb * P);
                }
                ++out[(size_t)(first_row + r) * P + q];
            }
    }
    bool once = true;
    for (int c : out) once = once && c == 1;
    CHECK(once);
}

static void routes() {
    for (int route = 0; route < 3; ++route)        // 0: L <= small_maxl, 1: four-step, 2: N = 4096
        for (int nb : {1, 2, 3, 8, 64})
            for (int K : {1, 2, 3, 4, 64, 128})
                for (long g_chunk : {1L, 2L, 3L, 8L, 100L, 4096L}) {
                    RouteCaps k;
                    k.n_cus = 256;  k.n_buoys = 3;
                    const int P = 3, W = K * 5;
                    RouteCall a;
                    a.n_windows = W;  a.n_pairs = P;  a.weighted = true;  a.integ = K;  a.n_bands = nb;  a.bounded = K > 1;
                    long cap = g_chunk;                                     // the largest chunk of real windows the plan may use
                    if (route == 2) {
                        k.generic = false;  k.chunk_windows = (int)g_chunk;
                    } else {
                        k.generic = true;  k.logL = route == 0 ? 9 : 14;  k.logL1 = route == 0 ? 0 : 5;  k.logL2 = k.logL - k.logL1;
                        k.small_maxl = 8192;  k.g_chunk = (int)g_chunk;  k.col_tile = 512;  k.cols_threads = 64;
                        const BandsPlan bp = plan_bands(g_chunk, W, nb, k.n_buoys, P, 1L << k.logL, route == 1, 0, 0, 0);
                        cap = bp.chunk;
                        CHECK(nb > 1 || cap == g_chunk);
                    }
                    const RoutePlan p = plan_route(k, a);
                    CHECK(p.route == (route == 2 ? kRoutePer4096 : route == 0 ? kRouteSmallL : kRouteFourStep));
                    const bool fits = cap / K >= 1;                         // a chunk of whole groups within the caps exists
                    CHECK((p.refused == kRefuseIntegChunk) == !fits);
                    if (!fits) {
                        CHECK(p.chunk == 0);
                        // the text names the bands only when they, not the ctx's own chunk, are what K does not fit
                        CHECK((p.bands_chunk > 0) == (route != 2 && nb > 1 && K > 1 && g_chunk >= K));
                        if (p.bands_chunk > 0) CHECK(p.bands_chunk == cap && p.bands_chunk < K);
                        continue;
                    }
                    CHECK(p.refused == kRouteOk);
                    CHECK(p.chunk >= K && p.chunk % K == 0 && p.chunk <= cap && p.chunk + K > cap);   // the largest such chunk
                    if (route != 2 && nb > 1) CHECK((long)p.chunk * nb <= kGenericMaxChunk);
                    if (route == 1 && nb > 1) CHECK((long)p.chunk * nb * P <= kMaxGridY);
                    replay(p, W, K, nb, P);
                }
    // the column-tile refusal applies as before, banded or not
    RouteCaps k;
    k.generic = true;  k.n_buoys = 3;  k.logL = 14;  k.logL1 = 5;  k.logL2 = 9;  k.small_maxl = 8192;  k.g_chunk = 64;
    k.col_tile = 16 * 64 + 1;  k.cols_threads = 64;  k.integ_max_per_thread = 16;
    RouteCall a;
    a.n_windows = 8;  a.n_pairs = 3;  a.weighted = true;  a.integ = 2;  a.n_bands = 3;
    CHECK(plan_route(k, a).refused == kRefuseIntegTile);
    a.integ = 1;
    CHECK(plan_route(k, a).refused == kRouteOk);
}

// check_request for grouped + banded: the staged rows, read to the last one
static void bounds_layout() {
    const int N = 64, B = 3, P = 3, K = 2, M = 3, W = 6, G = W / K;
    std::vector<float> iq(1);
    std::vector<int32_t> li((size_t)G * M * P);
    std::vector<float> lf(li.size()), pk(li.size());
    std::vector<double> bands((size_t)W * M * 2);
    for (int w = 0; w < W; ++w)
        for (int m = 0; m < M; ++m) {
            bands[((size_t)w * M + m) * 2] = -0.5 + 0.1 * m + 0.01 * w;
            bands[((size_t)w * M + m) * 2 + 1] = 0.1 * m + 0.02 * w;
        }
    RequestArgs a;
    a.n_buoys = B;  a.n_samples = N;  a.max_windows = W;
    a.grouped = true;  a.banded = true;  a.n_bands = M;  a.integrate = K;
    a.iq = iq.data();  a.n_windows = W;  a.n_pairs = 0;
    a.band_cps = bands.data();  a.band_per_window = 1;
    a.lag_int = li.data();  a.lag_frac = lf.data();  a.peak = pk.data();
    Request r;
    std::string err;
    // no bounds: the full interval per pair in the shared form -- one row serves every (group, band)
    CHECK(check_request(a, &r, &err) == RMX_OK);
    CHECK(r.integ == K && r.n_bands == M && r.bounded && !r.bounds_per_window && r.bound_rows == P);
    CHECK(r.bounds == r.own_bounds.data() && r.own_bounds.size() == 2 * (size_t)P);
    CHECK(r.bounds[2 * (P - 1)] == -(N - 1) && r.bounds[2 * (P - 1) + 1] == N - 1);
    CHECK(r.band_per_window && r.bins.size() == 2 + 2 * (size_t)W * M);     // [full band | one band set per REAL window]
    // shared bounds: the caller's array as it is
    std::vector<int32_t> shared = {-3, 3, -4, 4, -5, 5};
    a.lag_bounds = shared.data();
    CHECK(check_request(a, &r, &err) == RMX_OK);
    CHECK(r.bounds == shared.data() && r.bound_rows == P && !r.bounds_per_window);
    // per-group bounds: G * n_bands rows, group-major, each group's row once per band; exactly G rows of the caller's are read
    std::vector<int32_t> per_group((size_t)G * P * 2);
    for (int g = 0; g < G; ++g)
        for (int q = 0; q < P; ++q) {
            per_group[((size_t)g * P + q) * 2] = -(10 * g + q);
            per_group[((size_t)g * P + q) * 2 + 1] = 10 * g + q + 1;
        }
    a.lag_bounds = per_group.data();
    a.bounds_per_window = 1;
    CHECK(check_request(a, &r, &err) == RMX_OK);
    CHECK(r.bounds_per_window && r.bound_rows == (long)G * M * P && r.own_bounds.size() == (size_t)G * M * P * 2);
    for (int g = 0; g < G; ++g)
        for (int m = 0; m < M; ++m)
            for (int q = 0; q < P; ++q) {
                const size_t row = ((size_t)g * M + m) * P + q;             // the kernels' index: row (g * n_bands + m), pair q
                CHECK(r.bounds[2 * row] == -(10 * g + q) && r.bounds[2 * row + 1] == 10 * g + q + 1);
            }
    // a bad interval names the GROUP; a bad band names the REAL window
    per_group[((size_t)2 * P + 1) * 2] = 7;
    per_group[((size_t)2 * P + 1) * 2 + 1] = 6;
    CHECK(check_request(a, &r, &err) == RMX_E_INVAL && err.find("lag_bounds of group 2, pair 1") != std::string::npos);
    bands[((size_t)5 * M + 2) * 2] = 0.4;
    bands[((size_t)5 * M + 2) * 2 + 1] = 0.3;
    CHECK(check_request(a, &r, &err) == RMX_E_INVAL && err.find("band 2 of window 5") != std::string::npos);
    // the order: integrate in front of the NULL buffer, n_bands in front of the bands
    a.integrate = 4;
    a.band_cps = nullptr;
    CHECK(check_request(a, &r, &err) == RMX_E_INVAL && err.find("not a positive multiple of integrate = 4") != std::string::npos);
    a.integrate = K;
    CHECK(check_request(a, &r, &err) == RMX_E_INVAL && err == "NULL buffer");
    a.band_cps = bands.data();
    a.n_bands = 65;
    CHECK(check_request(a, &r, &err) == RMX_E_INVAL && err.find("n_bands 65") != std::string::npos);
    // the overlap text counts G * n_bands * P slots
    a.n_bands = M;
    bands[((size_t)5 * M + 2) * 2] = 0.1;
    per_group[((size_t)2 * P + 1) * 2] = -6;
    a.quality = pk.data();
    CHECK(check_request(a, &r, &err) == RMX_E_INVAL && err.find("quality overlaps peak") != std::string::npos);
    char want[64];
    std::snprintf(want, sizeof want, "the %d x 4 floats", G * M * P);
    CHECK(err.find(want) != std::string::npos);
    // integrate = 1 keeps the banded entry's layout: one row per virtual window
    a.quality = nullptr;
    a.integrate = 1;
    std::vector<int32_t> per_window((size_t)W * P * 2, 1);
    a.lag_bounds = per_window.data();
    std::vector<int32_t> li1((size_t)W * M * P);
    std::vector<float> lf1(li1.size()), pk1(li1.size());
    a.lag_int = li1.data();  a.lag_frac = lf1.data();  a.peak = pk1.data();
    CHECK(check_request(a, &r, &err) == RMX_OK && r.bound_rows == (long)W * M * P && r.own_bounds.size() == (size_t)W * M * P * 2);
}

int main() {
    routes();
    bounds_layout();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
