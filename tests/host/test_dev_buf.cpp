// The buffers of a ctx (radio-mapper_amd/csrc/dev_buf.hpp) on a counting malloc that fails on demand: ownership, the
// ledger, the waits, and the state every failed request leaves behind.  A CPU program, built with
// g++ -fsanitize=address,undefined and leak detection by tests/test_dev_buf_sanitized.py; no GPU, no HIP.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "../../radio-mapper_amd/csrc/dev_buf.hpp"

using namespace rmx::mem;

static int g_failed = 0;
#define CHECK(x)                                                              \
    do {                                                                      \
        if (!(x)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);        \
            ++g_failed;                                                       \
        }                                                                     \
    } while (0)

// the policy: malloc, counted; allocation number `fail_at` (device and pinned count together, from 1) fails, and so does
// any request above `max_bytes` -- the "device" has that much room for one block
struct Fake {
    int live = 0, allocs = 0, waits = 0, uploads = 0, refusals = 0, fail_at = 0, fail_upload_at = 0;
    size_t max_bytes = SIZE_MAX;
    void* grab(size_t bytes) {
        ++allocs;
        if (allocs == fail_at || bytes > max_bytes) return nullptr;
        ++live;
        return std::malloc(bytes);
    }
    void* alloc(size_t bytes) { return grab(bytes); }
    void free(void* p) { --live; std::free(p); }
    void* alloc_pinned(size_t bytes) { return grab(bytes); }
    void free_pinned(void* p) { --live; std::free(p); }
    bool upload(void* dst, const void* src, size_t bytes) {
        if (++uploads == fail_upload_at) return false;
        std::memcpy(dst, src, bytes);
        return true;
    }
    void wait() { ++waits; }
    void refused(const char*, size_t) { ++refusals; }
};
using A = Arena<Fake>;
template <class T> using Counted = Buf<T, Fake, kCounted>;
template <class T> using Uncounted = Buf<T, Fake, kUncounted>;
template <class T> using Pinned = Buf<T, Fake, kPinned>;

// ---- 1. any interleaving of reserve, assign, move and destruction: live blocks = non-empty buffers, ledger = counted bytes
struct Zoo {
    A* a;
    std::vector<std::unique_ptr<Counted<int>>> c;
    std::vector<std::unique_ptr<Uncounted<double>>> u;
    std::vector<std::unique_ptr<Pinned<char>>> p;
    explicit Zoo(A* arena) : a(arena), c(4), u(4), p(4) {}
    void check() const {
        int holding = 0;
        size_t counted = 0;
        for (auto& b : c) if (b) { holding += b->get() != nullptr; counted += b->bytes(); CHECK((b->get() != nullptr) == (b->capacity() > 0)); }
        for (auto& b : u) if (b) holding += b->get() != nullptr;
        for (auto& b : p) if (b) holding += b->get() != nullptr;
        CHECK(a->m.live == holding);
        CHECK(a->ledger == counted);
    }
};
template <class B, class T>
static void one_op(A* a, std::vector<std::unique_ptr<B>>& v, unsigned r, const std::vector<T>& src, bool can_assign) {
    std::unique_ptr<B>& b = v[r % 4];
    std::unique_ptr<B>& other = v[(r / 4) % 4];
    const size_t n = (r / 16) % 40;
    switch ((r / 1024) % 6) {
    case 0: if (!b) b.reset(new B(a)); break;
    case 1: b.reset(); break;                                                  // destruction
    case 2: if (b) (void)b->reserve(n); break;
    case 3:
        if (b && can_assign) {
            if constexpr (!std::is_same<B, Pinned<char>>::value) {
                if (b->assign(src.data(), n)) CHECK(n == 0 || std::memcmp(b->get(), src.data(), n * sizeof(T)) == 0);
            }
        }
        break;
    case 4: if (b && other && &b != &other) *b = std::move(*other); break;     // move assignment: other is left empty
    default: if (b) { std::unique_ptr<B> m(new B(std::move(*b))); b = std::move(m); } break;   // move construction
    }
}
static void test_interleavings() {
    for (int fail_every : {0, 7, 3}) {
        A a;
        {
            Zoo z(&a);
            std::vector<int> si(40, 5);
            std::vector<double> sd(40, 2.5);
            std::vector<char> sc(40, 'x');
            unsigned s = 12345u + (unsigned)fail_every;
            for (int k = 0; k < 20000; ++k) {
                s = s * 1664525u + 1013904223u;
                const unsigned r = s >> 8;
                a.m.fail_at = fail_every && (k % fail_every == 0) ? a.m.allocs + 1 : 0;   // the next allocation, if this op makes one
                switch (r % 3) {
                case 0: one_op(&a, z.c, r / 3, si, true); break;
                case 1: one_op(&a, z.u, r / 3, sd, true); break;
                default: one_op(&a, z.p, r / 3, sc, false); break;
                }
                z.check();
            }
        }
        CHECK(a.m.live == 0 && a.ledger == 0);   // everything destroyed
    }
}

// ---- 2. what a reserve costs
static void test_reserve_costs() {
    A a;
    Counted<float> b(&a);
    CHECK(b.reserve(100) && a.m.allocs == 1 && a.m.waits == 0);          // growing from nothing: no wait
    CHECK(a.ledger == 400);
    float* p = b.get();
    CHECK(b.reserve(100) && b.reserve(1) && b.reserve(0) && b.try_reserve(99));
    CHECK(a.m.allocs == 1 && a.m.waits == 0 && b.get() == p);            // within capacity: no allocation, no wait
    CHECK(b.reserve(101) && a.m.allocs == 2 && a.m.waits == 1);          // growing a held block: exactly one wait
    CHECK(a.ledger == 404 && a.m.live == 1);
    std::vector<float> v(200, 1.0f);
    CHECK(b.assign(v.data(), 50) && a.m.allocs == 2 && a.m.waits == 2);  // overwriting a block that stays: one wait
    CHECK(b.assign(v.data(), 200) && a.m.allocs == 3 && a.m.waits == 3); // growing: the release's wait only
    a.m.fail_at = a.m.allocs + 1;
    CHECK(!b.try_reserve(1000) && a.m.refusals == 0);                    // try_reserve keeps quiet ...
    CHECK(b.get() == nullptr && b.capacity() == 0 && a.ledger == 0 && a.m.live == 0);
    a.m.fail_at = a.m.allocs + 1;
    CHECK(!b.reserve(1000) && a.m.refusals == 1 && a.m.waits == 4);      // ... reserve reports; an empty buffer waits for nothing
    CHECK(b.reserve(10) && a.ledger == 40);
    a.m.fail_upload_at = a.m.uploads + 1;
    CHECK(!b.assign(v.data(), 5) && a.m.refusals == 2);                  // a failed upload: holds nothing either
    CHECK(b.get() == nullptr && b.capacity() == 0 && a.ledger == 0 && a.m.live == 0);
    Pinned<int32_t> h(&a);
    CHECK(h.reserve(8) && a.ledger == 0 && a.m.live == 1);               // pinned memory is never counted
}

// ---- 3. the n-th allocation fails, for every n ---------------------------------------------------------------------------
// A small ctx on the pattern of rmx_ctx: the pair plan in two buffers under one key, the pair list under the plan's pairs,
// a table under an int, two counted buffers and a stage.
struct PlanKey {
    std::vector<int32_t> pairs;
    int ppb = 0;
    bool operator==(const PlanKey& o) const { return ppb == o.ppb && pairs == o.pairs; }
};
struct Ctx {
    A a;
    Keyed<int64_t, Fake, PlanKey> items{&a};
    Keyed<int, Fake, PlanKey> part_begin{&a};
    Keyed<int32_t, Fake, std::vector<int32_t>> pair_list{&a};
    Keyed<float, Fake, int> table{&a};
    Counted<float> spec{&a}, stage_d{&a};
    Pinned<int32_t> stage_h{&a};
    Uncounted<char> in{&a};
    bool consistent() const {
        const int holding = (items.get() != nullptr) + (part_begin.get() != nullptr) + (pair_list.get() != nullptr) + (table.get() != nullptr) +
                            (spec.get() != nullptr) + (stage_d.get() != nullptr) + (stage_h.get() != nullptr) + (in.get() != nullptr);
        return a.m.live == holding && a.ledger == spec.bytes() + stage_d.bytes();
    }
};
// build_plan of rmx_hip.hip: a cache hit needs BOTH buffers under the key
static bool plan_hit(const Ctx& c, const PlanKey& k) { return c.items.holds(k) && c.part_begin.holds(k); }
static bool build_plan(Ctx& c, const PlanKey& k) {
    if (plan_hit(c, k)) return true;
    std::vector<int64_t> items(k.pairs.size() / 2, 7);
    std::vector<int> parts(k.pairs.size() / 2 / (size_t)k.ppb + 2, 3);
    return c.items.refill(k, items) && c.part_begin.refill(k, parts);
}
static bool fill_pairs(Ctx& c, const std::vector<int32_t>& pairs) {   // the tail of generic_ensure, ensure_ref_pairs
    if (c.pair_list.holds(pairs)) return true;
    return c.pair_list.refill(pairs, pairs);
}
static const PlanKey kPlanA{{0, 1, 0, 2, 1, 2}, 2}, kPlanB{{0, 2, 1, 2, 0, 1, 0, 3}, 1}, kPlanC{{0, 1}, 1};
// the script: each step names the keyed buffers it refills, so that the failing step can be judged
struct Step {
    const char* name;
    bool (*run)(Ctx&);
    bool (*matches_nothing)(const Ctx&);   // after a failure of this step
};
static const Step kScript[] = {
    {"spec", [](Ctx& c) { return c.spec.reserve(1000); }, [](const Ctx& c) { return c.spec.capacity() == 0; }},
    {"plan A", [](Ctx& c) { return build_plan(c, kPlanA); }, [](const Ctx& c) { return !plan_hit(c, kPlanA); }},
    {"pairs A", [](Ctx& c) { return fill_pairs(c, kPlanA.pairs); }, [](const Ctx& c) { return !c.pair_list.holds(kPlanA.pairs) && !c.pair_list.get(); }},
    {"stage", [](Ctx& c) { return c.stage_h.reserve(6) && c.stage_d.reserve(6); }, [](const Ctx& c) { return !c.stage_h.get() || !c.stage_d.get(); }},
    {"in", [](Ctx& c) { return c.in.reserve(64); }, [](const Ctx& c) { return c.in.capacity() == 0; }},
    {"table 9", [](Ctx& c) { std::vector<float> t(512, 1.f); return c.table.holds(9) || c.table.refill(9, t); }, [](const Ctx& c) { return !c.table.holds(9) && !c.table.holds(10); }},
    {"plan B", [](Ctx& c) { return build_plan(c, kPlanB); }, [](const Ctx& c) { return !plan_hit(c, kPlanA) && !plan_hit(c, kPlanB); }},
    {"pairs B", [](Ctx& c) { return fill_pairs(c, kPlanB.pairs); }, [](const Ctx& c) { return !c.pair_list.holds(kPlanA.pairs) && !c.pair_list.holds(kPlanB.pairs) && !c.pair_list.get(); }},
    {"spec grows", [](Ctx& c) { return c.spec.reserve(5000); }, [](const Ctx& c) { return c.spec.capacity() == 0; }},
    {"table 10", [](Ctx& c) { std::vector<float> t(1024, 2.f); return c.table.holds(10) || c.table.refill(10, t); }, [](const Ctx& c) { return !c.table.holds(9) && !c.table.holds(10); }},
    {"stage grows", [](Ctx& c) { return c.stage_h.reserve(60) && c.stage_d.reserve(60); }, [](const Ctx& c) { return !c.stage_h.get() || !c.stage_d.get(); }},
    {"plan A again", [](Ctx& c) { return build_plan(c, kPlanA); }, [](const Ctx& c) { return !plan_hit(c, kPlanA) && !plan_hit(c, kPlanB); }},
    {"plan C (smaller: no allocation)", [](Ctx& c) { return build_plan(c, kPlanC); }, [](const Ctx& c) { return !plan_hit(c, kPlanC); }},
};
static void test_every_nth_allocation_fails() {
    int total = 0;
    {
        Ctx c;
        for (const Step& s : kScript) { CHECK(s.run(c)); CHECK(c.consistent()); }
        total = c.a.m.allocs;
        CHECK(plan_hit(c, kPlanC) && c.items.get()[0] == 7 && c.part_begin.get()[0] == 3);
    }
    CHECK(total >= 12);
    for (int n = 1; n <= total; ++n) {
        Ctx c;
        c.a.m.fail_at = n;
        int failures = 0;
        for (const Step& s : kScript) {
            if (s.run(c)) { CHECK(c.consistent()); continue; }
            ++failures;
            CHECK(c.a.m.allocs == n);            // the failing allocation, nothing attempted behind it
            CHECK(s.matches_nothing(c));         // the failing buffer is empty and no key describes it
            CHECK(c.consistent());               // live blocks and ledger agree with the buffers
            CHECK(s.run(c));                     // the retry, same key: refilled
            CHECK(!s.matches_nothing(c) && c.consistent());
        }
        CHECK(failures == 1);
        CHECK(plan_hit(c, kPlanC) && c.items.get()[0] == 7 && c.table.holds(10) && c.table.get()[1023] == 2.f);
    }
}
// the two cases by name ---------------------------------------------------------------------------------------------------
// the cached key must not outlive the block it describes: the old plan's key went before its blocks did
static void test_plan_refill_second_allocation_fails() {
    Ctx c;
    CHECK(build_plan(c, kPlanA));
    c.a.m.fail_at = c.a.m.allocs + 2;            // items' new block is served, part_begin's is not
    CHECK(!build_plan(c, kPlanB));
    CHECK(c.items.holds(kPlanB) && !c.part_begin.holds(kPlanB) && c.part_begin.get() == nullptr && c.part_begin.capacity() == 0);
    CHECK(!plan_hit(c, kPlanA) && !plan_hit(c, kPlanB));   // the next call with the OLD pair list does not hit the cache
    CHECK(c.consistent());
    const int before = c.a.m.uploads;
    CHECK(build_plan(c, kPlanA) && c.a.m.uploads == before + 2);   // ... it fills both buffers again
    CHECK(plan_hit(c, kPlanA) && c.items.capacity() >= 3 && c.items.get()[2] == 7 && c.part_begin.get()[0] == 3);
}
static void test_pair_list_refill_fails() {
    Ctx c;
    CHECK(fill_pairs(c, kPlanA.pairs));
    c.a.m.fail_at = c.a.m.allocs + 1;
    CHECK(!fill_pairs(c, kPlanB.pairs));
    CHECK(c.pair_list.get() == nullptr && !c.pair_list.holds(kPlanA.pairs) && !c.pair_list.holds(kPlanB.pairs) && c.consistent());
    CHECK(fill_pairs(c, kPlanA.pairs) && c.pair_list.get() != nullptr);   // never a null list behind a matching key
    CHECK(std::memcmp(c.pair_list.get(), kPlanA.pairs.data(), kPlanA.pairs.size() * 4) == 0);
    // an upload that fails on a block that stays: the same end
    c.a.m.fail_upload_at = c.a.m.uploads + 1;
    CHECK(!fill_pairs(c, kPlanC.pairs) && c.pair_list.get() == nullptr && !c.pair_list.holds(kPlanC.pairs) && c.consistent());
}

// ---- 4. generic_ensure's rule: a failed chunk allocation releases every chunk-sized buffer, halves the chunk, retries
struct Chunked {
    A a;
    Counted<float> spec{&a}, spec_r{&a}, prod{&a};
    int chunk;
    bool ensure(size_t per_window, size_t prod_per_window) {
        for (;;) {
            const bool ok = spec.try_reserve((size_t)chunk * per_window) && prod.try_reserve((size_t)chunk * prod_per_window);
            if (ok) return true;
            spec.release();
            spec_r.release();
            prod.release();
            if (chunk <= 1) return false;
            chunk = (chunk + 1) / 2;
        }
    }
};
static void test_halve_and_retry() {
    for (int room : {64, 63, 33, 32, 17, 5, 2, 1}) {      // windows of the larger buffer the fake device can serve
        Chunked g;
        g.chunk = 64;
        g.a.m.max_bytes = (size_t)room * 100 * sizeof(float);
        CHECK(g.spec_r.reserve(10));                      // a chunk-sized buffer from an earlier call
        const bool whole = room >= 64;
        CHECK(g.ensure(50, 100));
        int want = 64;
        while (want > room) want = (want + 1) / 2;        // the first chunk of the halving sequence that fits
        CHECK(g.chunk == want);
        CHECK(g.spec.capacity() == (size_t)want * 50 && g.prod.capacity() == (size_t)want * 100);
        CHECK((g.spec_r.capacity() == 10) == whole);      // released with the others whenever the chunk changed
        CHECK(g.a.ledger == g.spec.bytes() + g.prod.bytes() + g.spec_r.bytes() && g.a.m.refusals == 0);
    }
    Chunked g;                                            // not even one window
    g.chunk = 8;
    g.a.m.max_bytes = 99 * sizeof(float);
    CHECK(!g.ensure(50, 100));
    CHECK(g.chunk == 1 && g.a.ledger == 0 && g.a.m.live == 0 && !g.spec.get() && !g.prod.get());
    g.a.m.max_bytes = SIZE_MAX;
    CHECK(g.ensure(50, 100) && g.chunk == 1 && g.a.ledger == 150 * sizeof(float));   // and the ctx stays usable
}

int main() {
    test_interleavings();
    test_reserve_costs();
    test_every_nth_allocation_fails();
    test_plan_refill_second_allocation_fails();
    test_pair_list_refill_fails();
    test_halve_and_retry();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
