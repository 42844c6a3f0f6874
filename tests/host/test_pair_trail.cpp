// host::plan_pair_trail (radio-mapper_amd/csrc/host_plan.hpp), the order in which k_win walks a window's pairs among buoys
// 1 .. B-1, without a GPU: built with g++ -fsanitize=address,undefined by tests/test_pair_trail_sanitized.py.  The checks
// replay what the kernel does with the table -- two register arrays, one request per step into the array the table names --
// and ask that each step then finds X_i and X_j where the table says they are, which for this kernel is X_i in array 0.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../radio-mapper_amd/csrc/host_plan.hpp"

using namespace rmx::host;

static int g_failed = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s (B = %d)\n", __FILE__, __LINE__, #cond, g_B); \
            ++g_failed;                                                         \
        }                                                                       \
    } while (0)
static int g_B = 0;

static void check_table(const PairTrail& t, int B) {
    g_B = B;
    const int M2 = (B - 1) * (B - 2) / 2;
    CHECK(t.n_buoys == B);
    CHECK((int)t.steps.size() == M2);
    CHECK((t.first_load >= 0) == (M2 > 0));
    std::vector<int> seen((size_t)B * B, 0);
    int arr[2] = {t.first_load, B - 1};   // phase 1 leaves X_{B-1} in array 1 and requests first_load into array 0
    int loads = 0, reloads = 0;
    for (int k = 0; k < M2; ++k) {
        const TrailStep& s = t.steps[k];
        CHECK(1 <= s.i && s.i < s.j && s.j <= B - 1);
        if (!(1 <= s.i && s.i < s.j && s.j <= B - 1)) return;
        ++seen[(size_t)s.i * B + s.j];
        CHECK(s.out_idx == s.i * B - s.i * (s.i + 1) / 2 + (s.j - s.i - 1));
        CHECK(s.xi_arr == 0 || s.xi_arr == 1);
        CHECK(s.load_arr == 0 || s.load_arr == 1);
        // the operands are where the table says
        CHECK(arr[s.xi_arr] == s.i && arr[1 - s.xi_arr] == s.j);
        if (k + 1 == M2) {
            CHECK(s.load_idx == -1 && !s.reload && s.load2 == -1);
            break;
        }
        const TrailStep& nx = t.steps[k + 1];
        CHECK(1 <= s.load_idx && s.load_idx <= B - 1);
        if (s.reload) {
            CHECK(1 <= s.load2 && s.load2 <= B - 1 && s.load2 != s.load_idx);
            arr[s.load_arr] = s.load_idx;
            arr[1 - s.load_arr] = s.load2;
            loads += 2;
            ++reloads;
        } else {
            CHECK(s.load2 == -1);
            // exactly one buoy is shared with the next step, it keeps its array, and the request overwrites the other one
            const int shared = (s.i == nx.i || s.i == nx.j) + (s.j == nx.i || s.j == nx.j);
            CHECK(shared == 1);
            const int keep = (s.i == nx.i || s.i == nx.j) ? s.i : s.j;
            const int keep_arr = keep == s.i ? s.xi_arr : 1 - s.xi_arr;
            const int keep_arr_next = keep == nx.i ? nx.xi_arr : 1 - nx.xi_arr;
            CHECK(keep_arr == keep_arr_next);
            CHECK(s.load_arr == 1 - keep_arr);             // the dropped array
            CHECK(s.load_idx == (keep == nx.i ? nx.j : nx.i));
            arr[s.load_arr] = s.load_idx;
            ++loads;
        }
    }
    for (int i = 1; i < B; ++i)
        for (int j = i + 1; j < B; ++j) CHECK(seen[(size_t)i * B + j] == 1);   // every pair exactly once
    CHECK(t.loads == loads && t.reloads == reloads);
    CHECK(t.sim_hits2 == trail_sim_hits(t, 2) && t.sim_hits3 == trail_sim_hits(t, 3));
    CHECK(t.sim_hits2 >= 0 && t.sim_hits2 <= t.sim_hits3 && t.sim_hits3 <= loads + (M2 > 0));
    if (M2 > 0) CHECK(t.steps[0].j == B - 1 && t.steps[0].xi_arr == 0);       // X_{B-1} resident in array 1
    // the planner's own stated minimum of steps that reload both arrays: none, at either parity of B
    CHECK(t.min_reloads == 0 && t.reloads == t.min_reloads);
    // one request per step but the last (B = 2 has no step, so nothing to request; with the request of phase 1's last
    // pair that is loads + 1 spectrum loads per window)
    CHECK(t.loads == (M2 > 0 ? M2 - 1 : 0));
    if (B == 8) CHECK(t.loads == 20);
    // what the kernel can walk: X_i in array 0 at every step (one copy of h1 per request target, none per role)
    CHECK(trail_kernel_ok(t));
    for (const TrailStep& s : t.steps) CHECK(s.xi_arr == 0 && s.reload == 0);
    // the kernel's copy
    const std::vector<int32_t> e = encode_pair_trail(t);
    CHECK((int)e.size() == 4 * (M2 + 1));
    if ((int)e.size() != 4 * (M2 + 1)) return;
    CHECK(e[0] == B - 2 && e[1] == 0);   // out_idx of (0, B-1); its request goes to array 0
    for (size_t k = 0; k < e.size() / 4; ++k) {
        CHECK(e[4 * k] >= 0 && e[4 * k] < B * (B - 1) / 2);
        CHECK(e[4 * k + 1] == 0 || e[4 * k + 1] == 1);
        CHECK(e[4 * k + 2] >= 0 && e[4 * k + 2] < B && e[4 * k + 3] == 0);   // requests stay inside the scratch
        if (k > 0) {
            const TrailStep& s = t.steps[k - 1];
            CHECK(e[4 * k] == s.out_idx && e[4 * k + 1] == s.load_arr);
            if (s.load_idx >= 0) CHECK(e[4 * k + 2] == s.load_idx);
        }
    }
    if (M2 > 0) CHECK(e[2] == t.first_load);
}

int main(int argc, char**) {
    const bool verbose = argc > 1;
    for (int B = 2; B <= 32; ++B) {
        const PairTrail t = plan_pair_trail(B);
        check_table(t, B);
        std::printf("B %2d: %3d steps, %3d requests (+1 from phase 1), %d reloads, LRU2 hits %2d, LRU3 hits %3d\n", B, (int)t.steps.size(),
                    t.loads, t.reloads, t.sim_hits2, t.sim_hits3);
        if (verbose && (B <= 9 || B == 16)) {
            std::printf("   first_load %d |", t.first_load);
            for (const TrailStep& s : t.steps) std::printf(" (%d,%d)->%c", s.i, s.j, s.load_arr ? 'b' : 'a');
            std::printf("\n");
        }
    }
    check_table(plan_pair_trail(40), 40);   // any buoy count: the construction has no size limit
    {   // an order the kernel cannot walk -- a pair with no buoy in common with the one before it, and X_i in array 1 -- is
        // recognised, and gets no device table
        PairTrail bad;
        trail_from_pairs(5, {{4, 1}, {2, 3}, {3, 4}, {2, 4}, {1, 2}, {1, 3}}, &bad);
        g_B = 5;
        CHECK(bad.reloads == 1 && !trail_kernel_ok(bad) && encode_pair_trail(bad).empty());
        PairTrail roles;
        trail_from_pairs(4, {{3, 1}, {1, 2}, {2, 3}}, &roles);   // (2,3): X_2 sits in array 1
        g_B = 4;
        CHECK(roles.reloads == 0 && roles.steps[2].xi_arr == 1 && !trail_kernel_ok(roles) && encode_pair_trail(roles).empty());
    }
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
