// host::plan_bands (radio-mapper_amd/csrc/host_plan.hpp), the buffer arithmetic of rmx_xcorr_batch_bands, without a GPU:
// built with g++ -fsanitize=address,undefined by tests/test_bands_plan_sanitized.py.  The checks replay what the launch
// code does with the plan -- allocate the stated bytes, then write every slot of every chunk -- so an index past an
// allocation is an AddressSanitizer report, not a wrong number.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../radio-mapper_amd/csrc/host_plan.hpp"

using namespace rmx::host;

static int g_failed = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            ++g_failed;                                                         \
        }                                                                       \
    } while (0)

// the launch code's walk over a call: chunks of plan.chunk real windows, each chunk's virtual slots written into buffers
// of exactly the stated sizes (one byte per 8-byte product element would do: elements, not bytes, are what may overrun)
static void replay(long g_chunk, int W, int nb, int B, int P, long L, bool four_step, long tiles, int logL1, size_t rec) {
    const BandsPlan bp = plan_bands(g_chunk, W, nb, B, P, L, four_step, tiles, logL1, rec);
    CHECK(bp.chunk >= 1 && bp.chunk <= (g_chunk < 1 ? 1 : g_chunk));
    CHECK(bp.vwindows == bp.chunk * nb && bp.slots == bp.vwindows * P);
    CHECK(bp.out_elems == (size_t)W * nb * P);
    if (nb == 1) CHECK(bp.chunk == (g_chunk < 1 ? 1 : g_chunk));
    std::vector<unsigned char> prod(bp.prod_bytes / 8), recs(bp.rec_bytes), halo(bp.halo_bytes / 4);
    std::vector<int> out(bp.out_elems, 0);
    for (long w0 = 0; w0 < W; w0 += bp.chunk) {
        const long wc = W - w0 < bp.chunk ? W - w0 : bp.chunk;
        const long slots = wc * nb * P;                       // generic_pairs: slots of this chunk
        CHECK(slots <= bp.slots);
        for (long s = 0; s < slots; ++s) {
            if (four_step) {
                prod[(size_t)s * L + (L - 1)] = 1;                                        // g_rows: the slot's last product element
                recs[((size_t)s * tiles + (tiles - 1)) * rec + (rec - 1)] = 1;            // g_cols_inv: its last tile record
                halo[(((size_t)s * tiles + (tiles - 1)) * 2 + 1) * ((size_t)1 << logL1) + (((size_t)1 << logL1) - 1)] = 1;
            }
            const long v = w0 * nb + s / P;                   // the virtual window, window-major
            CHECK(v / nb >= w0 && v / nb < w0 + wc);          // its real window lies in the chunk: the spectra are there
            ++out[(size_t)v * P + s % P];                     // g_final / the pair kernels: the output slot
        }
    }
    bool once = true;
    for (int c : out) once = once && c == 1;
    CHECK(once);                                              // every output slot written exactly once
}

int main() {
    // n_bands = 1 changes nothing: the chunk and the sizes generic_ensure had
    {
        const BandsPlan b = plan_bands(4096, 100, 1, 8, 28, 1L << 14, true, 8, 7, 16);
        CHECK(b.chunk == 4096 && b.slots == 4096L * 28);
        CHECK(b.prod_bytes == (size_t)4096 * 28 * (1 << 14) * 8);
        CHECK(b.rec_bytes == (size_t)4096 * 28 * 8 * 16);
        CHECK(b.halo_bytes == ((size_t)4096 * 28 * 8 * 2 * 4) << 7);
    }
    // the virtual windows of a chunk stay under the cap, the four-step slots under the grid's rows
    {
        const BandsPlan b = plan_bands(4096, 4096, 8, 3, 3, 1L << 14, false, 0, 0, 0);
        CHECK(b.chunk == 512 && b.vwindows == 4096 && b.prod_bytes == 0);
        const BandsPlan c = plan_bands(4096, 4096, 8, 8, 28, 1L << 14, true, 8, 7, 16);
        CHECK(c.slots <= kMaxGridY && c.chunk == kMaxGridY / (8 * 28));
        const BandsPlan d = plan_bands(4096, 4096, 64, 8, 28, 1L << 14, true, 8, 7, 16);
        CHECK(d.chunk == kMaxGridY / (64 * 28) && d.slots <= kMaxGridY);
    }
    // the byte budget shrinks the chunk: spectra + n_bands products per window
    {
        const long L = 1L << 22, per_win = (3 + 4 * 3) * L * 8;
        const BandsPlan b = plan_bands(64, 64, 4, 3, 3, L, true, 256, 10, 16, 8 * per_win);
        CHECK(b.chunk == 8 && b.prod_bytes == (size_t)8 * 4 * 3 * L * 8);
        const BandsPlan one = plan_bands(64, 64, 4, 3, 3, L, true, 256, 10, 16, per_win / 2);   // never below one window
        CHECK(one.chunk == 1 && one.slots == 12);
    }
    // degenerate arguments stay in range
    {
        const BandsPlan b = plan_bands(0, 0, 3, 3, 0, 32, false, 0, 0, 0);
        CHECK(b.chunk == 1 && b.slots == 0 && b.out_elems == 0);
        const BandsPlan c = plan_bands(5, -1, 0, 3, 3, 32, false, 0, 0, 0);
        CHECK(c.chunk == 5 && c.vwindows == 5 && c.out_elems == 0);
    }
    // the launch code's walk, over shapes with a seam, a remainder chunk and every band count at the limits
    for (int nb : {1, 2, 3, 8, 64})
        for (int W : {1, 2, 5, 9})
            for (long g_chunk : {1L, 2L, 4L, 4096L}) {
                replay(g_chunk, W, nb, 3, 3, 32, false, 0, 0, 0);                 // L <= small_maxl: outputs only
                replay(g_chunk, W, nb, 3, 4, 512, true, 2, 4, 16);                // four-step, custom pair list of 4
                replay(g_chunk, W, nb, 8, 28, 16384, true, 8, 7, 16);             // N = 8192, 8 buoys
            }
    // what plan_route hands the launch code is plan_bands' chunk, on both per-transform routes
    {
        RouteCaps k;
        k.generic = true;  k.n_buoys = 3;  k.logL = 14;  k.logL1 = 5;  k.logL2 = 9;  k.small_maxl = 8192;  k.g_chunk = 4096;  k.n_cus = 256;
        RouteCall a;
        a.n_windows = 4096;  a.n_pairs = 3;  a.weighted = true;  a.n_bands = 8;
        RoutePlan p = plan_route(k, a);
        CHECK(p.route == kRouteFourStep);
        CHECK(p.chunk == plan_bands(4096, 4096, 8, 3, 3, 1L << 14, true, 0, 0, 0).chunk && p.chunk * 8 <= kGenericMaxChunk);
        k.small_maxl = 16384;
        p = plan_route(k, a);
        CHECK(p.route == kRouteSmallL && p.chunk == 512);
        a.n_bands = 1;
        CHECK(plan_route(k, a).chunk == 4096);
        // N = 4096: the pairs-per-workgroup model sees the virtual windows
        RouteCaps k4;
        k4.n_cus = 256;  k4.n_buoys = 8;  k4.chunk_windows = 4096;
        RouteCall b;
        b.n_windows = 4;  b.n_pairs = 28;  b.weighted = true;
        int q1 = 0, q8 = 0;
        (void)split_cost4096(256, 8, 28, 4, 0, &q1);
        (void)split_cost4096(256, 8, 28, 32, 0, &q8);
        CHECK(plan_route(k4, b).ppb == q1);
        b.n_bands = 8;
        CHECK(plan_route(k4, b).ppb == q8 && plan_route(k4, b).route == kRoutePer4096);
    }
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
