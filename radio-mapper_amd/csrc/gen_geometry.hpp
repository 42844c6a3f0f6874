// gen_geometry.hpp -- the generic path's numbers, written down once: thread counts, the four-step split and the dynamic-LDS
// layout of every kernel of generic_path.hpp / win_eo.hpp / detect_path.hpp.  No HIP in here: the kernels take their region
// pointers from these layouts, rmx_hip.hip takes the byte counts of its launches from the same functions, and
// tests/host/test_gen_geometry.cpp compiles the header with g++ -fsanitize=address,undefined
// (tests/test_gen_geometry_sanitized.py) and holds every layout to the formulas the launch code used to carry.
//
// A layout names every region of a kernel's dynamic LDS as {offset, length, alignment} in BYTES, and two totals:
//   used   the end of the last region the kernel touches
//   bytes  what the host passes at the launch (and to hipFuncSetAttribute); never below `used`, sometimes above it --
//          LABNOTES.md (R20) lists every such slack; trimming one changes occupancy and is a measured change of its own
// ok() is the check both sides rely on: regions in order and disjoint (the one named overlay of the column kernels
// excepted), each aligned, used <= bytes <= kLdsMaxBytes.  Compile-time layouts static_assert it, generic_init refuses a
// ctx whose run-time layouts fail it (a byte count above 160 KiB that an option asks for is kept and left to
// hipFuncSetAttribute to refuse, as it always was).
// The kernels' instructions depend on HOW an offset is computed, not only on its value (the integer types, the order of
// the additions, whether a term folds in the front end): each region length below is therefore written the way the
// kernels have always computed it, is inlined with the kernels' own helpers (RMX_LEN), and tools/isa_diff.py holds a
// change of this file to "0 kernels differ".
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define RMX_HD __host__ __device__
#define RMX_LEN __host__ __device__ __attribute__((always_inline))   // a region length read inside a kernel: inlined with the kernel's own helpers
#else
#define RMX_HD
#define RMX_LEN
#endif

namespace rmx {
namespace gen {

constexpr int kGThreads = 256;
constexpr long kLdsMaxBytes = 160 * 1024;   // a CU's LDS (gfx950)

// threads per row of the row kernels: two threads per radix-16 group (the passes leave half of them idle, the
// streaming loops use all: measured better than one thread per group on the 2048-point rows of cfg2)
RMX_HD constexpr int rows_tpr(int R) { return (R >> 3) < kGThreads ? ((R >> 3) > 0 ? (R >> 3) : 1) : kGThreads; }
// LDS element index -> padded position: one complex of padding per 16 keeps the stride-16 accesses of the last
// fused passes (each thread walks 16 neighbouring elements) on distinct banks: lane i's element 16 i + m sits at
// 17 i + m, and 17 is odd.  Every access to a transform buffer goes through lp().
RMX_HD constexpr long lp(long e) { return e + (e >> 4); }
// the positions of the two padded layouts (LdsIO, LdsIOA<BM> of generic_path.hpp)
RMX_HD constexpr int lds_pos(int e) { return e + (e >> 4); }
RMX_HD constexpr int lds_pos_a(int e, int bm) { return e + ((e >> bm) << 4); }
// columns per tile: 16 (128-byte row segments), or 8 when L1 = 1024 so that two 64 KiB tiles share a CU and
// one workgroup's loads and stores overlap the other's butterflies (measured: cfg2 8.7 -> 8.1 ms)
RMX_HD constexpr int col_log_t(int l1) { return l1 >= 10 ? 3 : 4; }
// threads of a column kernel: one radix-16 work item per thread and pass, 64 .. 1024
RMX_HD constexpr int cols_threads(int l1, int log_t) {
    return ((1 << l1) << log_t) / 16 >= 1024 ? 1024 : (((1 << l1) << log_t) / 16 < 64 ? 64 : ((1 << l1) << log_t) / 16);
}
// threads of the small path (g_fwd_small / g_pair_small): one radix-16 group per thread and pass, 64 .. 1024
RMX_HD constexpr int small_threads(long L) { return (L >> 4) >= 1024 ? 1024 : ((L >> 4) < 64 ? 64 : (int)(L >> 4)); }
constexpr int kColTabPad = 1;   // the column kernels' per-column tables [na + nb + 1]: an odd stride (generic_path.hpp)

// g_rows_fused / g_win_fused: stages of the pass that meets `left` stages above the 16-point blocks
RMX_HD constexpr int fused_pass_m(int left) {
    return (left & 3) == 0 ? 4 : ((left & 3) == 1 && left > 1 ? 3 : (left & 3));
}
// Twiddles: every pass (block size 2^B, M stages) has its own table [k = 1 .. 2^M - 1][l < 2^(B-M)] =
// W_R^(l k 2^(LOGR-B)) in LDS, one behind the other from the first pass (B = LOGR) down; the inverse's passes are
// the forward's in reverse order and use the same tables conjugated.  Lanes read consecutive entries (the
// strided reads of a shared W_R table were 2..16-way bank conflicts: half of this kernel's LDS cycles).
RMX_HD constexpr int fused_tab_off(int logR, int B) {      // offset of pass B's table, in entries
    int cur = logR, acc = 0;
    while (cur > B) {
        const int M = fused_pass_m(cur - 4);
        acc += ((1 << M) - 1) << (cur - M);
        cur -= M;
    }
    return acc;
}
RMX_HD constexpr int fused_tab_total(int logR) { return fused_tab_off(logR, 4); }
// rows of 4096, default plan, at most 3 buoys: the passes' twiddles live in registers (FusedTw)
RMX_HD constexpr bool fused_tw_regs(int nb, int logR, bool def) { return def && logR == 12 && nb <= 3; }
// one transform buffer of those two kernels, in entries: the larger of its two layouts (lp() and, where the middle pass's
// blocks have 256 elements, the unit-stride layout A)
RMX_HD constexpr int fused_buf(int logR) {
    const int bm = logR - fused_pass_m(logR - 4), R = 1 << logR;
    const int pa = bm == 8 ? lds_pos_a(R, 8) : lds_pos(R);
    return lds_pos(R) > pa ? lds_pos(R) : pa;
}
template <int LOGR>
struct FusedPlan {
    static constexpr int M0 = fused_pass_m(LOGR - 4), BM = LOGR - M0, MM = BM - 4;      // first pass, middle pass
    static_assert(MM >= 1 && MM <= 4 && fused_pass_m(BM - 4) == MM, "rows of 2^9 .. 2^12: first pass, one middle pass, 16-point blocks");
    static constexpr bool kLayoutA = BM == 8;   // the unit-stride layout where its blocks line up with lp()'s; rows of 512 keep lp()
    static constexpr int buf = fused_buf(LOGR);
};

// ---- layouts ---------------------------------------------------------------------------------------------------
struct Region {
    long off, len;   // bytes
    int align;       // of the region's element type: 8 float2, 16 float4, 4 float / int / unsigned, 2, 1
    RMX_HD constexpr long end() const { return off + len; }
    RMX_HD constexpr bool aligned() const { return off % align == 0; }
};
// regions in order, disjoint and aligned; used <= bytes <= the CU's LDS
RMX_HD constexpr bool regions_ok(long used, long bytes, long at) { return at <= used && used <= bytes && bytes <= kLdsMaxBytes; }
template <class... R>
RMX_HD constexpr bool regions_ok(long used, long bytes, long at, Region r, R... rest) {
    return r.off >= at && r.len >= 0 && r.aligned() && regions_ok(used, bytes, r.end(), rest...);
}

// A run-time layout is a sequence of regions, one behind the other from offset 0.  Each struct below states every
// region's LENGTH once, as a static function in the unit and the integer type the kernels index that region with
// ("entries": float2, 8 bytes; "words": 4 bytes), so that a kernel walks from region to region with exactly the
// arithmetic it always had; the *_layout() function next to it sums the same lengths into byte offsets for the host and
// for the checks.  x_off: the transform buffer(s) start every layout.

// g_fwd_small (pair = false: the transform alone) and g_pair_small / pair_small_integ: L padded complex, then the
// workgroup argmax's value word and index word per thread
struct SmallLds {
    static constexpr long x_off = 0;
    static RMX_LEN constexpr size_t x_bytes(long L) { return (size_t)lp(L) * 8; }
    static RMX_LEN constexpr int sv_words(int nthr) { return nthr; }
    static RMX_LEN constexpr int sk_words(int nthr) { return nthr; }
    Region x, sv, sk;
    long used, bytes;
    RMX_HD constexpr bool ok() const { return regions_ok(used, bytes, 0, x, sv, sk); }
};
RMX_HD constexpr SmallLds small_layout(long L, int nthr, bool pair) {
    SmallLds s{};
    s.x = Region{SmallLds::x_off, (long)SmallLds::x_bytes(L), 8};
    s.sv = Region{s.x.end(), pair ? SmallLds::sv_words(nthr) * 4L : 0, 4};
    s.sk = Region{s.sv.end(), pair ? SmallLds::sk_words(nthr) * 4L : 0, 4};
    s.used = s.bytes = s.sk.end();
    return s;
}
// what generic_init lets every small-path kernel use: the pair kernel's layout at the largest thread count
RMX_HD constexpr long small_allow_bytes(long L) { return small_layout(L, 1024, true).bytes; }

// g_rows (fwd: the forward rows; else the inverse rows) and g_rows_anchor (the inverse layout at the default threads per
// row): rpw = 256 / tpr rows of R padded complex | inverse: per row the W_L factor tables T1[2^a] T2[R / 2^a], a = logR / 2
// | the W_R half table | inverse rows with 8 < logR < 12: the q = 16 pass's own table [15][16]
struct RowsLds {
    static constexpr long x_off = 0;
    static RMX_LEN constexpr long row_entries(int R) { return lp(R); }
    static RMX_LEN constexpr long x_entries(int R, int rpw) { return (long)rpw * lp(R); }
    static RMX_LEN constexpr int t_row_entries(int logR, int R) { return (1 << (logR >> 1)) + (R >> (logR >> 1)); }
    template <bool TW>   // (the direction as a template argument: the kernels' arithmetic then folds where it always did)
    static RMX_LEN constexpr long t_entries(int logR, int R, int rpw) { return TW ? (long)rpw * ((1 << (logR >> 1)) + (R >> (logR >> 1))) : 0; }
    static RMX_LEN constexpr int twl_entries(int R) { return R >> 1; }
    // the inverse's q = 16 pass has its own table for rows of 2^(kOwn16Above + 1) .. 2^(kOwn16Below - 1)
    // (rows of 4096 go without: three workgroups of 52 KiB share a CU, and 2 KiB more make it two -- 5.46 -> 5.88 ms)
    static constexpr int kOwn16Above = 8, kOwn16Below = 12, kTw16Entries = 240;
    static RMX_HD constexpr bool own16(bool fwd, int logR) { return !fwd && logR > kOwn16Above && logR < kOwn16Below; }
    Region x, t, twl, tw16;
    long used, bytes;
    RMX_HD constexpr bool ok() const { return regions_ok(used, bytes, 0, x, t, twl, tw16); }
};
RMX_HD constexpr RowsLds rows_layout(int logR, int tpr, bool fwd) {
    const int R = 1 << logR, rpw = kGThreads / tpr, a = logR >> 1, n1 = 1 << a, n2 = R >> a;
    RowsLds s{};
    s.x = Region{RowsLds::x_off, RowsLds::x_entries(R, rpw) * 8, 8};
    s.t = Region{s.x.end(), (fwd ? RowsLds::t_entries<false>(logR, R, rpw) : RowsLds::t_entries<true>(logR, R, rpw)) * 8, 8};
    s.twl = Region{s.t.end(), RowsLds::twl_entries(R) * 8L, 8};
    s.tw16 = Region{s.twl.end(), RowsLds::own16(fwd, logR) ? RowsLds::kTw16Entries * 8L : 0, 8};
    s.used = s.tw16.end();
    // every row kernel of a ctx is launched with ONE count: the inverse's table room, and 240 entries below 4096-point rows
    s.bytes = ((long)rpw * (lp(R) + n1 + n2) + (long)(R >> 1) + (R < 4096 ? 240 : 0)) * 8;
    return s;
}

// g_cols_fwd, g_cols_inv, cols_inv_integ: the tile [L1][T] (forward: flat; inverse: padded by lp()) | forward: T
// per-column tables [na + nb + 1], na = 2^(l1 / 2), nb = L1 / na | the W_L1 half table.  The inverse kernels have no
// per-column tables and put the argmax words of their (at most 16) waves where the tables would be: the overlay sv / sk.
struct ColsLds {
    static constexpr long x_off = 0;
    static RMX_LEN constexpr long x_entries(int L1, int log_t) { return lp((long)L1 << log_t); }
    static RMX_LEN constexpr long tab_entries(int l1, int L1, int log_t) { return (long)(1 << log_t) * ((1 << (l1 >> 1)) + (L1 >> (l1 >> 1)) + kColTabPad); }
    static RMX_LEN constexpr int twl_entries(int L1) { return L1 >> 1; }
    static constexpr int kSvWords = 16, kSkWords = 16;
    Region x, tab, twl;
    Region sv, sk;             // overlay, inside tab
    long used, bytes;
    RMX_HD constexpr bool ok() const {
        return regions_ok(used, bytes, 0, x, tab, twl) && sv.off == tab.off && sv.aligned() && sk.off == sv.end() && sk.aligned() &&
               sk.end() <= tab.end();
    }
};
RMX_HD constexpr ColsLds cols_layout(int l1, int log_t) {
    const int L1 = 1 << l1;
    ColsLds s{};
    s.x = Region{ColsLds::x_off, ColsLds::x_entries(L1, log_t) * 8, 8};
    s.tab = Region{s.x.end(), ColsLds::tab_entries(l1, L1, log_t) * 8, 8};
    s.twl = Region{s.tab.end(), ColsLds::twl_entries(L1) * 8L, 8};
    s.sv = Region{s.tab.off, ColsLds::kSvWords * 4, 4};
    s.sk = Region{s.sv.end(), ColsLds::kSkWords * 4, 4};
    s.used = s.bytes = s.twl.end();
    return s;
}

// g_rows_fused: upw = 256 / (R / 16) transform buffers | per unit the W_L factor tables T1 T2 | the passes' twiddle
// tables (none when they live in registers)
struct FusedLds {
    static constexpr long x_off = 0;
    static RMX_LEN constexpr int upw(int logR) { return kGThreads / (((1 << logR) >> 4) > 0 ? ((1 << logR) >> 4) : 1); }
    static RMX_LEN constexpr int buf_entries(int logR) { return fused_buf(logR); }
    static RMX_LEN constexpr int x_entries(int logR) { return upw(logR) * fused_buf(logR); }
    static RMX_LEN constexpr int t_row_entries(int logR) { return (1 << (logR >> 1)) + ((1 << logR) >> (logR >> 1)); }
    static RMX_LEN constexpr int t_entries(int logR) { return upw(logR) * t_row_entries(logR); }
    static RMX_LEN constexpr int tab_entries(int logR, bool tw_regs) { return tw_regs ? 0 : fused_tab_total(logR); }
    Region x, t, tab;
    long used, bytes;
    RMX_HD constexpr bool ok() const { return regions_ok(used, bytes, 0, x, t, tab); }
};
RMX_HD constexpr FusedLds fused_layout(int logR, bool tw_regs) {
    FusedLds s{};
    s.x = Region{FusedLds::x_off, FusedLds::x_entries(logR) * 8L, 8};
    s.t = Region{s.x.end(), FusedLds::t_entries(logR) * 8L, 8};
    s.tab = Region{s.t.end(), FusedLds::tab_entries(logR, tw_regs) * 8L, 8};
    s.used = s.bytes = s.tab.end();
    return s;
}

// g_win_fused: the transform buffers | the passes' twiddle tables (none when in registers) | eight argmax values, eight
// indices (one per wave and window: at most four of each are used)
struct WFusedLds {
    static constexpr long x_off = 0;
    static RMX_LEN constexpr int buf_entries(int logR) { return fused_buf(logR); }
    static RMX_LEN constexpr int x_entries(int logR) { return FusedLds::x_entries(logR); }
    static RMX_LEN constexpr int tab_entries(int logR, bool tw_regs) { return tw_regs ? 0 : fused_tab_total(logR); }
    static constexpr int kSvWords = 8, kSkWords = 8;
    Region x, tab, sv, sk;
    long used, bytes;
    RMX_HD constexpr bool ok() const { return regions_ok(used, bytes, 0, x, tab, sv, sk); }
};
RMX_HD constexpr WFusedLds wfused_layout(int logR, bool tw_regs) {
    WFusedLds s{};
    s.x = Region{WFusedLds::x_off, WFusedLds::x_entries(logR) * 8L, 8};
    s.tab = Region{s.x.end(), WFusedLds::tab_entries(logR, tw_regs) * 8L, 8};
    s.sv = Region{s.tab.end(), WFusedLds::kSvWords * 4, 4};
    s.sk = Region{s.sv.end(), WFusedLds::kSkWords * 4, 4};
    s.used = s.bytes = s.sk.end();
    return s;
}

// g_win_scr<LOGR>: geometry, pass tables and LDS of the whole-window kernel (generic_path.hpp has the kernel's story).
// LDS: upw windows of R padded complex | the passes' tables | 16 argmax values, 16 indices
template <int LOGR>
struct WinPlan {
    static constexpr int R = 1 << LOGR, tpr = R >> 4;
    static constexpr int ML = ((LOGR - 1) & 3) + 1, RADL = 1 << ML, NITL = 16 / RADL;   // the neighbour pass
    static constexpr int NP = (LOGR - ML) / 4;                                            // radix-16 passes, blocks LOGR, LOGR - 4, ..
    static constexpr int kTwRegFrom = 9, kTwGlobalFrom = 99;
    static constexpr bool TW1REG = LOGR >= kTwRegFrom && LOGR < kTwGlobalFrom;                  // first pass's twiddles in registers
    static constexpr bool TW1GLOBAL = LOGR >= kTwGlobalFrom;                            // ... or read from the global table
    static constexpr bool TW2REG = false;                                                 // the second pass's too: settled off
    static constexpr int thr = tpr < kGThreads ? kGThreads : tpr, upw = thr / tpr;         // threads, windows per workgroup
    static constexpr int tab_off(int b) {                                                 // entries in front of pass b's LDS table
        int acc = 0;
        for (int c = LOGR; c > b; c -= 4)
            if (!(c == LOGR && (TW1REG || TW1GLOBAL)) && !(c == LOGR - 4 && TW2REG)) acc += 15 << (c - 4);
        return acc;
    }
    static constexpr int tab_total = tab_off(ML);
    static constexpr long x_stride = lp(R) * 8;
    static constexpr Region x{0, (long)upw * lp(R) * 8, 8};
    static constexpr Region tab{x.end(), (long)tab_total * 8, 8};
    static constexpr Region sv{tab.end(), 16 * 4, 4};
    static constexpr Region sk{sv.end(), 16 * 4, 4};
    static constexpr size_t used = (size_t)sk.end(), lds_bytes = used;
    static_assert(regions_ok((long)used, (long)lds_bytes, 0, x, tab, sv, sk), "g_win_scr's LDS");
};

// g_win_scr14 and g_win_eo15: one 16384-point transform, 512 threads x two butterflies per pass (16 x 16 x 16 x 4): the
// padded buffer | the tables of the passes over blocks of 2^10 and 2^6 | 16 argmax values, 16 indices
struct Win14Lds {
    static constexpr int off10 = 0, off6 = 15 * 64, tab_total = 15 * 64 + 15 * 4;   // entries into tab
    static constexpr Region x{0, lp(16384) * 8, 8};
    static constexpr Region tab{x.end(), (long)tab_total * 8, 8};
    static constexpr Region sv{tab.end(), 16 * 4, 4};
    static constexpr Region sk{sv.end(), 16 * 4, 4};
    static constexpr size_t used = (size_t)sk.end(), bytes = used;
    static_assert(regions_ok((long)used, (long)bytes, 0, x, tab, sv, sk), "g_win_scr14's / g_win_eo15's LDS");
};

// det::d_fft_db: the whole window, padded
struct DetFftLds {
    static constexpr long x_off = 0;
    Region x;
    long used, bytes;
    RMX_HD constexpr bool ok() const { return regions_ok(used, bytes, 0, x); }
};
RMX_HD constexpr DetFftLds det_fft_layout(int N) {
    DetFftLds s{};
    s.x = Region{DetFftLds::x_off, lp(N) * 8, 8};
    s.used = s.bytes = s.x.end();
    return s;
}
// det::d_peaks: the dB spectrum [N] float | a state byte per bin | [N / 2] candidate positions (16 bit) | the radix
// select's histogram [256] | 8 scalars | one scan word per thread
struct DetPeaksLds {
    static constexpr long p_off = 0;
    static RMX_LEN constexpr int p_words(int N) { return N; }
    static RMX_LEN constexpr int st_bytes(int N) { return N; }
    static RMX_LEN constexpr int cand_halfwords(int N) { return N / 2; }
    static constexpr int kHistWords = 256, kBcWords = 8;
    static RMX_LEN constexpr int scan_words(int nthr) { return nthr; }
    Region p, st, cand, hist, bc, scan;
    long used, bytes;
    RMX_HD constexpr bool ok() const { return regions_ok(used, bytes, 0, p, st, cand, hist, bc, scan); }
};
RMX_HD constexpr DetPeaksLds det_peaks_layout(int N, int nthr) {
    DetPeaksLds s{};
    s.p = Region{DetPeaksLds::p_off, DetPeaksLds::p_words(N) * 4L, 4};
    s.st = Region{s.p.end(), (long)DetPeaksLds::st_bytes(N), 1};
    s.cand = Region{s.st.end(), DetPeaksLds::cand_halfwords(N) * 2L, 2};
    s.hist = Region{s.cand.end(), DetPeaksLds::kHistWords * 4, 4};
    s.bc = Region{s.hist.end(), DetPeaksLds::kBcWords * 4, 4};
    s.scan = Region{s.bc.end(), DetPeaksLds::scan_words(nthr) * 4L, 4};
    s.used = s.bytes = s.scan.end();
    return s;
}
constexpr int kDetMaxN = 16384;   // rmx_detect_batch's longest window
RMX_HD constexpr int det_fft_threads(int N) { return N >= 4096 ? 1024 : (N >= 1024 ? 256 : 64); }
RMX_HD constexpr int det_peaks_threads(int N) { return N >= 4096 ? 1024 : 256; }
// what rmx_detect_batch lets the two kernels use, whatever the window length
constexpr long kDetFftAllowBytes = det_fft_layout(kDetMaxN).bytes;
constexpr long kDetPeaksAllowBytes = kDetMaxN * 6 + 8192;
static_assert(det_fft_layout(kDetMaxN).ok() && det_peaks_layout(kDetMaxN, det_peaks_threads(kDetMaxN)).ok() &&
                  det_peaks_layout(kDetMaxN, det_peaks_threads(kDetMaxN)).bytes <= kDetPeaksAllowBytes && kDetPeaksAllowBytes <= kLdsMaxBytes,
              "the detect kernels' LDS at the longest window");

// ---- the geometry of one ctx -----------------------------------------------------------------------------------
// Everything the generic path's launches derive from (n_buoys, n_samples, options), computed once by generic_init.
// Knobs: anything with get(key, long*) and get_or(key, long) (host::Knobs).
struct Geometry {
    int n_buoys = 0, logL = 0;
    long small_maxl = 0;          // option small_maxl: the largest L that runs as one LDS transform per workgroup
    bool small = false;           // L <= small_maxl: g_fwd_small / g_pair_small; else the four-step kernels
    int small_threads = 0;
    size_t small_fwd_lds = 0, small_pair_lds = 0, small_allow_lds = 0;
    size_t wfused_lds[2] = {0, 0};   // g_win_fused [default plan] (2..4 buoys, 512 <= L <= 4096; else 0)
    // four-step (0 on the small path): L = L1 x L2, W_L^m = hi[m >> lo_bits] lo[m & (2^lo_bits - 1)]
    int logL1 = 0, logL2 = 0, lo_bits = 0;
    int col_log_t = 0, cols_threads = 0, rows_tpr = 0;
    int col_tiles = 0;            // L2 / columns per tile: the column kernels' grid.x, one tile record each
    long col_tile = 0;            // elements of a tile
    size_t cols_lds = 0, rows_lds = 0;
    size_t fused_lds[2] = {0, 0};    // g_rows_fused [default plan] (<= 4 buoys, rows of 2^9 .. 2^12; else 0)
    bool layouts_ok = true;       // every layout above passed ok() but for the 160 KiB bound, which stays the runtime's to refuse
};
template <class L>
RMX_HD constexpr bool layout_sound(const L& l) { return l.used <= l.bytes && (l.bytes > kLdsMaxBytes || l.ok()); }

template <class Knobs>
inline Geometry make_geometry(int n_buoys, int n_samples, const Knobs& knobs) {
    Geometry g;
    g.n_buoys = n_buoys;
    int logn = 0;
    while ((1 << logn) < n_samples) ++logn;
    g.logL = logn + 1;
    const long L = 1L << g.logL;
    // windows up to this zero-padded length run with the whole transform in LDS (128 KiB of the 160)
    // (L = 16384 -- N = 8192, the reference's iq_stream_client capture length -- is better off in the four-step path: one
    // 128 KiB transform per CU leaves nothing to overlap with; 0.77 -> 0.60 ms for 3 buoys x 1024 windows)
    g.small_maxl = knobs.get_or("small_maxl", 8192L);
    g.small = L <= g.small_maxl;
    long v = 0;
    if (g.small) {
        g.small_threads = gen::small_threads(L);
        g.small_fwd_lds = (size_t)small_layout(L, g.small_threads, false).bytes;
        g.small_pair_lds = (size_t)small_layout(L, g.small_threads, true).bytes;
        g.small_allow_lds = (size_t)small_allow_bytes(L);
        g.layouts_ok = layout_sound(small_layout(L, g.small_threads, true));
        if (n_buoys >= 2 && n_buoys <= 4 && g.logL >= 9 && g.logL <= 12)
            for (int d = 0; d < 2; ++d) {
                const WFusedLds w = wfused_layout(g.logL, d == 1 && fused_tw_regs(n_buoys, g.logL, true));
                g.wfused_lds[d] = (size_t)w.bytes;
                g.layouts_ok = g.layouts_ok && layout_sound(w);
            }
        return g;
    }
    // columns of length L1 <= 1024 (a tile of 16 columns is L1*128 bytes of LDS), rows of L2 = L/L1 <= 8192
    // columns a little shorter than rows (measured: 512 x 4096 beats 1024 x 2048 at L = 2^21, 256 x 2048 beats
    // 512 x 1024 at 2^19), rows at most 8192 (64 KiB of LDS)
    g.logL1 = (g.logL - 3) / 2;
    if (g.logL == 18) g.logL1 = 8;   // (measured: 256 x 1024 beats 128 x 2048 by 5 %)
    if (g.logL1 < g.logL - 13) g.logL1 = g.logL - 13;
    if (g.logL1 > 10) g.logL1 = 10;
    if (knobs.get("logl1", &v) && v >= 4 && v <= 10 && g.logL - v <= 13 && g.logL - v >= 4) g.logL1 = (int)v;
    g.logL2 = g.logL - g.logL1;
    g.lo_bits = (g.logL + 1) / 2;
    const int R = 1 << g.logL2;
    g.col_log_t = (int)knobs.get_or("col_logt", col_log_t(g.logL1));
    g.cols_threads = knobs.get("cols_threads", &v) ? (int)v : cols_threads(g.logL1, g.col_log_t);
    g.rows_tpr = rows_tpr(R);
    if (knobs.get("rows_tpr", &v) && v >= 1 && v <= kGThreads && (v & (v - 1)) == 0 && v <= R) g.rows_tpr = (int)v;
    g.col_tiles = R >> g.col_log_t;
    g.col_tile = (1L << g.logL1) << g.col_log_t;
    const ColsLds cl = cols_layout(g.logL1, g.col_log_t);
    const RowsLds rf = rows_layout(g.logL2, g.rows_tpr, true), ri = rows_layout(g.logL2, g.rows_tpr, false);
    g.cols_lds = (size_t)cl.bytes;
    g.rows_lds = (size_t)ri.bytes;
    g.layouts_ok = layout_sound(cl) && layout_sound(rf) && layout_sound(ri);
    if (n_buoys <= 4 && g.logL2 >= 9 && g.logL2 <= 12)
        for (int d = 0; d < 2; ++d) {
            const FusedLds f = fused_layout(g.logL2, d == 1 && fused_tw_regs(n_buoys, g.logL2, true));
            g.fused_lds[d] = (size_t)f.bytes;
            g.layouts_ok = g.layouts_ok && layout_sound(f);
        }
    return g;
}

}  // namespace gen
}  // namespace rmx
