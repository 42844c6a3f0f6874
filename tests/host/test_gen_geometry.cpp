// The generic path's geometry and LDS layouts (radio-mapper_amd/csrc/gen_geometry.hpp) under AddressSanitizer + UBSan.
// Built and run by tests/test_gen_geometry_sanitized.py:  g++ -std=c++17 -O1 -g -fsanitize=address,undefined
// -fno-sanitize-recover=all -o ... tests/host/test_gen_geometry.cpp ; exit code 0 = every check passed and neither
// sanitizer reported anything.
//
// namespace parent holds, verbatim, the byte-count formulas and the geometry rules the launch code (rmx_hip.hip) carried
// before this header existed, with the options map in place of the ctx.  The header is held to them over the whole
// domain the selection code can reach: `bytes` is what was launched then, bit for bit.
#include <cstdio>
#include <cstdlib>

#include "../../radio-mapper_amd/csrc/gen_geometry.hpp"
#include "../../radio-mapper_amd/csrc/host_plan.hpp"

using namespace rmx;
using rmx::host::Knobs;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

// ---- the parent's formulas, verbatim ----------------------------------------------------------------------------
namespace parent {
constexpr int kGThreads = 256;
constexpr int rows_tpr(int R) { return (R >> 3) < kGThreads ? ((R >> 3) > 0 ? (R >> 3) : 1) : kGThreads; }
constexpr long lp(long e) { return e + (e >> 4); }
constexpr int col_log_t(int l1) { return l1 >= 10 ? 3 : 4; }
constexpr int fused_pass_m(int left) { return (left & 3) == 0 ? 4 : ((left & 3) == 1 && left > 1 ? 3 : (left & 3)); }
constexpr int fused_tab_off(int logR, int B) {
    int cur = logR, acc = 0;
    while (cur > B) {
        const int M = fused_pass_m(cur - 4);
        acc += ((1 << M) - 1) << (cur - M);
        cur -= M;
    }
    return acc;
}
constexpr int fused_tab_total(int logR) { return fused_tab_off(logR, 4); }
constexpr bool fused_tw_regs(int nb, int logR, bool def) { return def && logR == 12 && nb <= 3; }
// FusedPlan<LOGR>::buf: the larger of LdsIO::pos(R) and IOA::pos(R), IOA = LdsIOA<8> where BM == 8, else LdsIO
static int fused_plan_buf(int logR) {
    const int M0 = fused_pass_m(logR - 4), BM = logR - M0, e = 1 << logR;
    const int pos_io = e + (e >> 4), pos_ioa = BM == 8 ? e + ((e >> 8) << 4) : pos_io;
    return pos_io > pos_ioa ? pos_io : pos_ioa;
}
static long gen_small_max_l(const Knobs& c) { return c.get_or("small_maxl", 8192L); }
static int gen_small_threads(long L) { const long t = L >> 4; return t >= 1024 ? 1024 : (t < 64 ? 64 : (int)t); }
static int gen_rows_tpr(const Knobs& c, int R) {
    int t = rows_tpr(R);
    long v;
    if (c.get("rows_tpr", &v) && v >= 1 && v <= kGThreads && (v & (v - 1)) == 0 && v <= R) t = (int)v;
    return t;
}
static size_t gen_rows_lds(const Knobs& c, int R) {
    const int tpr = gen_rows_tpr(c, R);
    int logR = 0;
    while ((1 << logR) < R) ++logR;
    const int a = logR >> 1;
    return ((size_t)(kGThreads / tpr) * ((size_t)lp(R) + (1 << a) + (R >> a)) + (size_t)(R >> 1) + (R < 4096 ? 240 : 0)) * 8;
}
static size_t gen_wfused_lds(int logR, bool tw_regs) {
    const int tpr = (1 << logR) >> 4, upw = kGThreads / tpr;
    return ((size_t)upw * fused_plan_buf(logR) + (size_t)(tw_regs ? 0 : fused_tab_total(logR)) + 8) * 8;
}
static size_t gen_fused_lds(int R, bool tw_regs = false) {
    int logR = 0;
    while ((1 << logR) < R) ++logR;
    const int a = logR >> 1, tpr = R >> 4, upw = kGThreads / (tpr > 0 ? tpr : 1);
    return ((size_t)upw * ((size_t)fused_plan_buf(logR) + (1 << a) + (R >> a)) + (size_t)(tw_regs ? 0 : fused_tab_total(logR))) * 8;
}
static int host_col_log_t(const Knobs& c, int l1) { return (int)c.get_or("col_logt", col_log_t(l1)); }
static size_t gen_cols_lds(const Knobs& c, int l1) {
    const int a = l1 >> 1, T = 1 << host_col_log_t(c, l1);
    return ((size_t)lp((long)(1 << l1) * T) + (size_t)T * ((1 << a) + ((1 << l1) >> a) + 1) + (size_t)((1 << l1) >> 1)) * 8;
}
static int gen_cols_threads(const Knobs& c, int l1) {
    const long work = (((long)1 << l1) << host_col_log_t(c, l1)) / 16;
    long v;
    if (c.get("cols_threads", &v)) return (int)v;
    return work >= 1024 ? 1024 : (work < 64 ? 64 : (int)work);
}
// WinPlan<LOGR>::lds_bytes with its table sizes spelt out: the first pass's twiddles in registers from log2 L = 9 on, a
// table of 15 << (c - 4) entries for every later radix-16 pass over blocks of 2^c
static size_t win_plan_lds(int logR) {
    const int R = 1 << logR, tpr = R >> 4, thr = tpr < kGThreads ? kGThreads : tpr, upw = thr / tpr, ML = ((logR - 1) & 3) + 1;
    int tab_total = 0;
    for (int c = logR - 4; c > ML; c -= 4) tab_total += 15 << (c - 4);
    return ((size_t)upw * lp(R) + tab_total + 16) * 8;
}
constexpr size_t kWinEoLds = ((size_t)lp(16384) + 15 * 64 + 15 * 4 + 16) * 8;   // g_win_scr14's literal and win_eo.hpp's constant
// generic_init's split and the ctx fields it filled
struct Init {
    int logL = 0, logL1 = 0, logL2 = 0, lo_bits = 0;
    bool small = false;
};
static Init generic_init(const Knobs& c, int n_samples) {
    Init g;
    int logn = 0;
    while ((1 << logn) < n_samples) ++logn;
    g.logL = logn + 1;
    const long L = 1L << g.logL;
    if (L <= gen_small_max_l(c)) {
        g.small = true;
        return g;
    }
    g.logL1 = (g.logL - 3) / 2;
    if (g.logL == 18) g.logL1 = 8;
    if (g.logL1 < g.logL - 13) g.logL1 = g.logL - 13;
    if (g.logL1 > 10) g.logL1 = 10;
    { long v; if (c.get("logl1", &v) && v >= 4 && v <= 10 && g.logL - v <= 13 && g.logL - v >= 4) g.logL1 = (int)v; }
    g.logL2 = g.logL - g.logL1;
    g.lo_bits = (g.logL + 1) / 2;
    return g;
}
}  // namespace parent

static const long kMax = 163840;
static long g_over = 0;   // layouts whose parent byte count exceeds the CU's LDS: recorded, the value kept

// regions in order, disjoint and aligned; used <= bytes == the parent's; bytes <= 160 KiB wherever the parent's is
template <class Lay>
static void check_layout(const Lay& lay, size_t parent_bytes, std::initializer_list<gen::Region> regions, const char* what, int a, int b) {
    long at = 0;
    for (const gen::Region& r : regions) {
        CHECK(r.off >= at && r.len >= 0);
        CHECK(r.off % r.align == 0);
        at = r.end();
    }
    CHECK(at <= lay.used);
    CHECK(lay.used <= lay.bytes);
    CHECK((size_t)lay.bytes == parent_bytes);
    if ((long)parent_bytes <= kMax) {
        CHECK(lay.bytes <= kMax);
        CHECK(lay.ok());
        CHECK(gen::layout_sound(lay));
    } else {
        if (g_over++ < 12) std::printf("over 160 KiB (kept, the runtime refuses it): %s(%d, %d) = %zu bytes\n", what, a, b, parent_bytes);
        CHECK(!lay.ok());
        CHECK(gen::layout_sound(lay));   // still sound: only the bound fails
    }
}

static Knobs knobs_of(std::initializer_list<std::pair<const char*, long>> kv) {
    Knobs k;
    for (const auto& e : kv) k.v[e.first] = e.second;
    return k;
}

static void test_rows() {
    for (int logR = 4; logR <= 13; ++logR) {
        const int R = 1 << logR, a = logR >> 1, n1 = 1 << a, n2 = R >> a;
        for (int tpr = 1; tpr <= 256; tpr <<= 1) {
            if (tpr > R) continue;   // the option admits powers of two up to min(256, R)
            const Knobs k = knobs_of({{"rows_tpr", tpr}});
            CHECK(parent::gen_rows_tpr(k, R) == tpr);
            const size_t pb = parent::gen_rows_lds(k, R);
            const long rpw = 256 / tpr;
            for (int fwd = 0; fwd < 2; ++fwd) {
                const gen::RowsLds l = gen::rows_layout(logR, tpr, fwd != 0);
                check_layout(l, pb, {l.x, l.t, l.twl, l.tw16}, fwd ? "rows_fwd" : "rows_inv", logR, tpr);
                // the kernels' former carve, entry for entry
                CHECK(l.x.off == 0 && gen::RowsLds::row_entries(R) == parent::lp(R) && l.x.len == rpw * parent::lp(R) * 8);
                CHECK(l.twl.off == (rpw * parent::lp(R) + (fwd ? 0 : rpw * (n1 + n2))) * 8 && l.twl.len == (R >> 1) * 8);
                CHECK(l.tw16.off == l.twl.off + (R >> 1) * 8);
                if (!fwd) CHECK(l.t.off == rpw * parent::lp(R) * 8 && gen::RowsLds::t_row_entries(logR, R) == n1 + n2 && l.t.len == rpw * (n1 + n2) * 8);
                if (fwd) CHECK(l.t.len == 0);
                CHECK((l.tw16.len == 240 * 8) == (!fwd && logR > 8 && logR < 12) && (l.tw16.len == 0 || l.tw16.len == 240 * 8));
            }
        }
        if (logR >= 9) {   // g_rows_anchor: compiled for rows of 2^9 .. 2^13 at the default threads per row
            const gen::RowsLds l = gen::rows_layout(logR, gen::rows_tpr(R), false);
            check_layout(l, parent::gen_rows_lds(Knobs{}, R), {l.x, l.t, l.twl, l.tw16}, "rows_anchor", logR, gen::rows_tpr(R));
            CHECK(l.ok());
        }
    }
}

static void test_cols() {
    for (int l1 = 3; l1 <= 10; ++l1)
        for (int lt = 3; lt <= 5; ++lt) {
            const Knobs k = knobs_of({{"col_logt", lt}});
            const gen::ColsLds l = gen::cols_layout(l1, lt);
            check_layout(l, parent::gen_cols_lds(k, l1), {l.x, l.tab, l.twl}, "cols", l1, lt);
            const long L1 = 1L << l1, T = 1L << lt, a = l1 >> 1, na = 1L << a, nb = L1 >> a;
            CHECK(l.tab.off == parent::lp(L1 << lt) * 8 && gen::kColTabPad == 1 && l.tab.len == T * (na + nb + 1) * 8);
            CHECK(l.twl.off == (parent::lp(L1 << lt) + T * (na + nb + 1)) * 8 && l.twl.len == (L1 >> 1) * 8);
            // the overlay of the inverse kernels: 16 + 16 words at the head of the table region, and inside it
            CHECK(l.sv.off == l.tab.off && l.sv.len == 64 && l.sk.off == l.sv.off + 64 && l.sk.len == 64);
            CHECK(l.sk.end() <= l.tab.end() && l.sv.off % 4 == 0 && l.sk.off % 4 == 0);
            CHECK(gen::cols_threads(l1, lt) == parent::gen_cols_threads(k, l1));
        }
    for (int l1 = 0; l1 <= 10; ++l1) CHECK(gen::col_log_t(l1) == parent::col_log_t(l1));
}

static void test_fused() {
    for (int logR = 9; logR <= 12; ++logR)
        for (int nb = 2; nb <= 4; ++nb)
            for (int twr = 0; twr < 2; ++twr) {
                const gen::FusedLds f = gen::fused_layout(logR, twr != 0);
                check_layout(f, parent::gen_fused_lds(1 << logR, twr != 0), {f.x, f.t, f.tab}, "rows_fused", logR, twr);
                const gen::WFusedLds w = gen::wfused_layout(logR, twr != 0);
                check_layout(w, parent::gen_wfused_lds(logR, twr != 0), {w.x, w.tab, w.sv, w.sk}, "win_fused", logR, twr);
                const long upw = 256 / ((1 << logR) >> 4), buf = parent::fused_plan_buf(logR), a = logR >> 1, n12 = (1L << a) + ((1L << logR) >> a);
                CHECK(gen::fused_buf(logR) == buf && gen::FusedLds::buf_entries(logR) == buf && gen::WFusedLds::buf_entries(logR) == buf && gen::FusedLds::upw(logR) == upw);
                CHECK(f.t.off == upw * buf * 8 && gen::FusedLds::t_row_entries(logR) == n12 && f.tab.off == upw * (buf + n12) * 8);
                CHECK(w.tab.off == upw * buf * 8 && w.sv.off == (upw * buf + (twr ? 0 : parent::fused_tab_total(logR))) * 8 && w.sk.off == w.sv.off + 32);
                CHECK(gen::fused_tw_regs(nb, logR, true) == parent::fused_tw_regs(nb, logR, true) && !gen::fused_tw_regs(nb, logR, false));
                CHECK(gen::fused_tab_total(logR) == parent::fused_tab_total(logR));
            }
}

template <int LOGR>
static void test_win_plan() {
    using P = gen::WinPlan<LOGR>;
    CHECK(P::lds_bytes == parent::win_plan_lds(LOGR) && P::used <= P::lds_bytes && (long)P::lds_bytes <= kMax);
    CHECK(P::x.off == 0 && P::tab.off == P::x.end() && P::sv.off == P::tab.end() && P::sk.off == P::sv.off + 64 && P::sk.end() == (long)P::used);
    CHECK(P::x.off % 8 == 0 && P::tab.off % 8 == 0 && P::sv.off % 4 == 0 && P::sk.off % 4 == 0);
    CHECK(P::x.len == P::upw * parent::lp(1 << LOGR) * 8 && P::x_stride == parent::lp(1 << LOGR) * 8);
}
static void test_win() {
    test_win_plan<9>();
    test_win_plan<10>();
    test_win_plan<11>();
    test_win_plan<12>();
    test_win_plan<13>();
    test_win_plan<14>();   // (g_win_scr<14>: option wscr14 = 0)
    // log2 L = 14 (g_win_scr14) and 15 (g_win_eo15: 16384-point halves): one definition for the two former literals
    using W = gen::Win14Lds;
    CHECK(W::bytes == parent::kWinEoLds && W::used <= W::bytes && (long)W::bytes <= kMax);
    CHECK(W::x.off == 0 && W::x.len == parent::lp(16384) * 8 && W::tab.off == W::x.end() && W::tab.len == (15 * 64 + 15 * 4) * 8);
    CHECK(W::sv.off == W::tab.end() && W::sk.off == W::sv.off + 64 && W::sk.end() == (long)W::used && W::off10 == 0 && W::off6 == 15 * 64);
}

static void test_small() {
    for (long L = 32; L <= 16384; L <<= 1) {
        const int sthr = parent::gen_small_threads(L);
        CHECK(gen::small_threads(L) == sthr);
        const gen::SmallLds f = gen::small_layout(L, sthr, false), p = gen::small_layout(L, sthr, true);
        check_layout(f, (size_t)parent::lp(L) * 8, {f.x, f.sv, f.sk}, "small_fwd", (int)L, sthr);
        check_layout(p, (size_t)parent::lp(L) * 8 + (size_t)sthr * 8, {p.x, p.sv, p.sk}, "small_pair", (int)L, sthr);
        CHECK(p.sv.off == parent::lp(L) * 8 && p.sk.off == p.sv.off + sthr * 4 && p.sk.len == sthr * 4);
        CHECK((size_t)gen::small_allow_bytes(L) == (size_t)parent::lp(L) * 8 + 1024 * 8 && gen::small_allow_bytes(L) >= p.bytes &&
              gen::small_allow_bytes(L) <= kMax);
    }
}

static void test_detect() {
    for (int N = 16; N <= 16384; N <<= 1) {
        const int fthr = N >= 4096 ? 1024 : (N >= 1024 ? 256 : 64), pthr = N >= 4096 ? 1024 : 256;
        CHECK(gen::det_fft_threads(N) == fthr && gen::det_peaks_threads(N) == pthr);
        const gen::DetFftLds f = gen::det_fft_layout(N);
        check_layout(f, (size_t)parent::lp(N) * 8, {f.x}, "d_fft_db", N, fthr);
        const gen::DetPeaksLds p = gen::det_peaks_layout(N, pthr);
        check_layout(p, (size_t)N * 4 + N + (size_t)N + 256 * 4 + 8 * 4 + (size_t)pthr * 4, {p.p, p.st, p.cand, p.hist, p.bc, p.scan}, "d_peaks", N, pthr);
        CHECK(p.st.off == 4L * N && p.cand.off == 5L * N && p.hist.off == 6L * N && p.bc.off == 6L * N + 1024 && p.scan.off == 6L * N + 1056);
        CHECK(f.bytes <= gen::kDetFftAllowBytes && p.bytes <= gen::kDetPeaksAllowBytes);
    }
    CHECK((size_t)gen::kDetFftAllowBytes == (size_t)parent::lp(16384) * 8 && gen::kDetPeaksAllowBytes == 16384 * 6 + 8192);
    CHECK(gen::kDetFftAllowBytes <= kMax && gen::kDetPeaksAllowBytes <= kMax);
}

// make_geometry against the parent's generic_init and launch-site lookups
static long g_geo_over = 0, g_geo_cases = 0;
static void check_geometry(int nb, int n_samples, const Knobs& k) {
    ++g_geo_cases;
    const parent::Init pi = parent::generic_init(k, n_samples);
    const gen::Geometry g = gen::make_geometry(nb, n_samples, k);
    const long L = 1L << pi.logL;
    CHECK(g.n_buoys == nb && g.logL == pi.logL && g.small == pi.small && g.small_maxl == parent::gen_small_max_l(k));
    CHECK(g.logL1 == pi.logL1 && g.logL2 == pi.logL2 && g.lo_bits == pi.lo_bits);
    bool over = false;
    if (pi.small) {
        const int sthr = parent::gen_small_threads(L);
        CHECK(g.small_threads == sthr && g.small_fwd_lds == (size_t)parent::lp(L) * 8 && g.small_pair_lds == (size_t)parent::lp(L) * 8 + (size_t)sthr * 8);
        CHECK(g.small_allow_lds == (size_t)parent::lp(L) * 8 + 1024 * 8 && (long)g.small_allow_lds <= kMax);
        CHECK(g.col_tiles == 0 && g.cols_lds == 0 && g.rows_lds == 0 && g.fused_lds[0] == 0 && g.fused_lds[1] == 0);
        if (nb >= 2 && nb <= 4 && pi.logL >= 9 && pi.logL <= 12) {   // pick_generic_kernels' condition for g_win_fused
            CHECK(g.wfused_lds[0] == parent::gen_wfused_lds(pi.logL, false));
            CHECK(g.wfused_lds[1] == parent::gen_wfused_lds(pi.logL, parent::fused_tw_regs(nb, pi.logL, true)));
            CHECK((long)g.wfused_lds[0] <= kMax && (long)g.wfused_lds[1] <= kMax);
        } else {
            CHECK(g.wfused_lds[0] == 0 && g.wfused_lds[1] == 0);
        }
    } else {
        const int l1 = pi.logL1, l2 = pi.logL2, lt = parent::host_col_log_t(k, l1);
        CHECK(l1 >= 3 && l1 <= 10 && l2 >= 4 && l2 <= 13);   // the domain the layout tests above cover
        CHECK(g.col_log_t == lt && g.cols_threads == parent::gen_cols_threads(k, l1) && g.rows_tpr == parent::gen_rows_tpr(k, 1 << l2));
        CHECK(g.col_tiles == (1 << l2) >> lt && g.col_tile == (1L << l1) << lt);
        CHECK(g.cols_lds == parent::gen_cols_lds(k, l1) && g.rows_lds == parent::gen_rows_lds(k, 1 << l2));
        over = (long)g.cols_lds > kMax || (long)g.rows_lds > kMax;
        if (nb <= 4 && l2 >= 9 && l2 <= 12) {   // pick_generic_kernels' condition for g_rows_fused
            CHECK(g.fused_lds[0] == parent::gen_fused_lds(1 << l2));
            CHECK(g.fused_lds[1] == parent::gen_fused_lds(1 << l2, parent::fused_tw_regs(nb, l2, true)));
            CHECK((long)g.fused_lds[0] <= kMax && (long)g.fused_lds[1] <= kMax);
        } else {
            CHECK(g.fused_lds[0] == 0 && g.fused_lds[1] == 0);
        }
        CHECK(g.small_threads == 0 && g.small_fwd_lds == 0 && g.wfused_lds[0] == 0);
    }
    CHECK(g.layouts_ok);   // used <= bytes and alignment everywhere; the 160 KiB bound is the runtime's to refuse
    if (over && g_geo_over++ < 12) {
        long a = -1, b = -1, c = -1;   // (-1: unset)
        k.get("col_logt", &a), k.get("rows_tpr", &b), k.get("logl1", &c);
        std::printf("over 160 KiB (kept): n_samples %d, col_logt %ld rows_tpr %ld logl1 %ld: cols %zu rows %zu bytes\n", n_samples, a, b, c, g.cols_lds,
                    g.rows_lds);
    }
}
static void test_geometry() {
    struct Opt { const char* key; long lo, hi; };
    const Opt maxl{"small_maxl", 256, 16384};
    const Opt others[] = {{"logl1", 4, 10}, {"col_logt", 3, 5}, {"rows_tpr", 1, 1024}, {"cols_threads", 64, 1024}};
    for (const host::OptionSpec& s : host::option_specs()) {   // lowest and highest are the option table's
        if (std::string(s.key) == maxl.key) CHECK(s.lo == maxl.lo && s.hi == maxl.hi);
        for (const Opt& o : others)
            if (std::string(s.key) == o.key) CHECK(s.lo == o.lo && s.hi == o.hi);
    }
    const int buoys[] = {2, 3, 4, 5, 8};
    for (int logn = 4; logn <= 22; ++logn)
        for (int nb : buoys)
            for (int m = 0; m < 3; ++m) {                      // small_maxl unset / lowest / highest ...
                Knobs base;
                if (m) base.v[maxl.key] = m == 1 ? maxl.lo : maxl.hi;
                check_geometry(nb, 1 << logn, base);
                for (const Opt& o : others)                    // ... times each other option at its lowest and highest
                    for (int e = 0; e < 2; ++e) {
                        Knobs k = base;
                        k.v[o.key] = e ? o.hi : o.lo;
                        check_geometry(nb, 1 << logn, k);
                    }
            }
    // rows_tpr = 1024 is above what the row kernels admit and falls back to the default; its largest admitted value too
    for (int logn = 8; logn <= 22; ++logn) check_geometry(3, 1 << logn, knobs_of({{"small_maxl", 256}, {"rows_tpr", 256}}));
}

// the cases of tests/test_gpu_option_geometry.py: used <= bytes <= 160 KiB before any of them runs on a GPU
static void test_gpu_cases() {
    struct Case { int n; const char* key; long v; };
    const Case cases[] = {{256, "col_logt", 3}, {256, "rows_tpr", 4}, {256, "logl1", 4}, {2048, "col_logt", 5}, {2048, "rows_tpr", 64}, {2048, "cols_threads", 128}};
    for (const Case& cs : cases) {
        const Knobs k = knobs_of({{"small_maxl", 256}, {cs.key, cs.v}});
        const gen::Geometry g = gen::make_geometry(3, cs.n, k);
        CHECK(!g.small && g.layouts_ok);
        const gen::ColsLds cl = gen::cols_layout(g.logL1, g.col_log_t);
        const gen::RowsLds rf = gen::rows_layout(g.logL2, g.rows_tpr, true), ri = gen::rows_layout(g.logL2, g.rows_tpr, false);
        CHECK(cl.ok() && rf.ok() && ri.ok());
        CHECK(cl.used <= cl.bytes && cl.bytes <= kMax && ri.used <= ri.bytes && rf.used <= rf.bytes && ri.bytes <= kMax);
        long v = 0;
        CHECK(k.get(cs.key, &v));
        if (std::string(cs.key) == "col_logt") CHECK(g.col_log_t == cs.v);
        if (std::string(cs.key) == "rows_tpr") CHECK(g.rows_tpr == cs.v);
        if (std::string(cs.key) == "logl1") CHECK(g.logL1 == cs.v);
        if (std::string(cs.key) == "cols_threads") CHECK(g.cols_threads == cs.v);
        std::printf("gpu case N %d %s %ld: L1 2^%d x L2 2^%d, tile 2^%d, %d col threads, %d per row, cols %zu rows %zu fused %zu / %zu bytes\n", cs.n, cs.key,
                    cs.v, g.logL1, g.logL2, g.col_log_t, g.cols_threads, g.rows_tpr, g.cols_lds, g.rows_lds, g.fused_lds[0], g.fused_lds[1]);
    }
}

int main() {
    test_rows();
    test_cols();
    test_fused();
    test_win();
    test_small();
    test_detect();
    test_geometry();
    test_gpu_cases();
    std::printf("%ld layouts and %ld of %ld geometries carry a parent byte count above 160 KiB (kept as they were)\n", g_over, g_geo_over, g_geo_cases);
    std::printf("all checks passed\n");
    return 0;
}
