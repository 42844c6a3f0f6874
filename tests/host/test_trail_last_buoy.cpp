// k_win does not store X_{B-1}: it stays in register array 1 behind phase 1, and its slot of the workgroup's scratch is
// never written.  So no entry of the kernel's table (host::encode_pair_trail), the padding behind the last step included,
// may name buoy B-1 as its request, and host::trail_kernel_ok must refuse a table that does.  Without a GPU: built with
// g++ -fsanitize=address,undefined by tests/test_trail_last_buoy_sanitized.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../radio-mapper_amd/csrc/host_plan.hpp"

using namespace rmx::host;

static int g_failed = 0;
static int g_B = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s (B = %d)\n", __FILE__, __LINE__, #cond, g_B); \
            ++g_failed;                                                         \
        }                                                                       \
    } while (0)

static void check_table(int B) {
    g_B = B;
    const PairTrail t = plan_pair_trail(B);
    const int M2 = (B - 1) * (B - 2) / 2;
    CHECK(trail_kernel_ok(t));
    const std::vector<int32_t> e = encode_pair_trail(t);
    CHECK((int)e.size() == 4 * (M2 + 1));
    if ((int)e.size() != 4 * (M2 + 1)) return;
    for (size_t k = 0; k < e.size() / 4; ++k) {
        const int req = e[4 * k + 2];
        CHECK(req != B - 1);            // never the spectrum that is not stored
        CHECK(req >= 0 && req < B);     // inside the scratch
        // wherever the kernel issues the request (B > 2: every entry, the padding included), phase 1 stored that spectrum
        if (M2 > 0) CHECK(1 <= req && req <= B - 2);
    }
    if (M2 > 0) {
        CHECK(t.first_load != B - 1);
        CHECK(t.steps.back().load_idx == -1 && e[4 * M2 + 2] == 1);   // the padding behind the last step: buoy 1
        for (const TrailStep& s : t.steps) CHECK(s.load_idx != B - 1);
    } else {
        CHECK(t.first_load == -1 && e[2] == 0);                       // B = 2: nothing stored, nothing requested
    }
}

int main() {
    for (int B = 2; B <= 32; ++B) check_table(B);
    check_table(40);
    // a table altered to request buoy B-1 is refused and gets no device copy: in a step, and as phase 1's own request
    for (int B : {3, 4, 5, 8, 9, 32, 40}) {
        g_B = B;
        PairTrail t = plan_pair_trail(B);
        CHECK(trail_kernel_ok(t) && !t.steps.empty());
        if (t.steps.empty()) continue;
        {
            PairTrail a = t;
            a.first_load = B - 1;
            CHECK(!trail_kernel_ok(a) && encode_pair_trail(a).empty());
        }
        for (size_t k = 0; k < t.steps.size(); ++k) {
            PairTrail a = t;
            a.steps[k].load_idx = B - 1;
            CHECK(!trail_kernel_ok(a) && encode_pair_trail(a).empty());
        }
    }
    {   // an order that comes back to B-1 after leaving it requests X_{B-1}: (1,3) (1,2) (2,3) at B = 4
        g_B = 4;
        PairTrail back;
        trail_from_pairs(4, {{3, 1}, {1, 2}, {2, 3}}, &back);
        CHECK(back.steps[1].load_idx == 3 && !trail_kernel_ok(back) && encode_pair_trail(back).empty());
    }
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
