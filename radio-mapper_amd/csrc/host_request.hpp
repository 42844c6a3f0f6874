// host_request.hpp -- what the caller of ONE correlation or Doppler-search entry asked for: the raw arguments in, every
// refusal of include/rmx.h in its promised order with its text, and the small host arrays the launch code stages out.
// As host_plan.hpp's plan_route says "which kernels run", check_request says "what was asked"; it reads no device and no
// ctx state beyond n_buoys, n_samples and max_windows.  No HIP in here: rmx_hip.hip includes it, and
// tests/host/test_request.cpp compiles it with g++ -fsanitize=address,undefined (tests/test_request_sanitized.py).
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rmx.h"
#include "host_plan.hpp"

namespace rmx {
namespace host {

// The arguments of one call as the caller passed them, and which entry family it came through.
struct RequestArgs {
    int n_buoys = 0, n_samples = 0, max_windows = 0;   // of the ctx
    bool grouped = false;           // the entries that take `integrate` (_integrated, _refined, _quality)
    bool banded = false;            // rmx_xcorr_batch_bands(_quality, _integrated), rmx_caf_batch_bands: band_cps is [..][n_bands][2] and never NULL
    int n_bands = 0;                // as passed to a banded entry (0 from the single-band entries)
    bool bounds_required = false;   // rmx_xcorr_batch_bounded: lag_bounds is never NULL
    const void* iq = nullptr;
    int n_windows = 0;
    const int32_t* pairs = nullptr;
    int n_pairs = 0;
    int integrate = 1;
    const double* band_cps = nullptr;
    int band_per_window = 0;        // (bands_per_window of the banded entries)
    unsigned weighting = RMX_WEIGHT_NONE;
    const int32_t* lag_bounds = nullptr;
    int bounds_per_window = 0;      // (bounds_per_group of the grouped entries)
    int refine = 0;
    int32_t* lag_int = nullptr;
    float *lag_frac = nullptr, *peak = nullptr, *quality = nullptr;
    unsigned flags = 0;             // RMX_IN_DEVICE, RMX_OUT_DEVICE, RMX_IN_U8: which pointers the kernels themselves touch
    // the Doppler search (check_caf_request): the grid, and its two outputs in front of the three above
    const double* doppler_cps = nullptr;
    int n_dopplers = 0;
    int32_t* dop_idx = nullptr;
    float* dop_frac = nullptr;      // or NULL: not computed
};

// The checked request in host form.  The plain call allocates nothing: bins and own_bounds stay empty.
struct Request {
    int n_pairs = 0;                // resolved: the default list's length where pairs == NULL
    bool empty = false;             // return RMX_OK, write nothing
    bool weighted = false;          // bins go to the device.  False for a full band (or none) without weighting: the plain call
    bool phat = false;
    bool bounded = false;           // bounds go to the device.  False only when every interval is full and integrate == 1
    int n_bands = 1;                // > 1: bins is [full band | band set]; 1 IS the weighted request
    int integ = 1, refine = 0;
    std::vector<int32_t> bins;      // signed bins [lo, hi]: one row, or one per window; banded: the full band, then
                                    // [n_bands] rows, or [n_windows][n_bands]
    bool band_per_window = false;   // the rows (the band sets) are per window
    const int32_t* bounds = nullptr;   // [bound_rows][2]: the caller's array, or own_bounds
    long bound_rows = 0;
    bool bounds_per_window = false;    // one row of n_pairs intervals per window (group, virtual window), else one for all
    std::vector<int32_t> own_bounds;   // the full interval per pair (integrated call without bounds); each window's row
                                       // (group's) row n_bands times, window-major (banded call with per-window bounds)
};

// *err = the text; returns RMX_E_INVAL.  (512 bytes: what rmx_last_error has always kept of a text)
#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline int refuse(std::string* err, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *err = buf;
    return RMX_E_INVAL;
}

inline int check_n_windows(int n_windows, int max_windows, std::string* err) {
    if (n_windows < 0 || n_windows > max_windows) return refuse(err, "n_windows %d not in 0..max_windows=%d", n_windows, max_windows);
    return RMX_OK;
}
// the shape of a batch: n_windows in range; pairs == NULL is the default list, and *n_pairs becomes its length
inline int check_batch(int n_buoys, int max_windows, int n_windows, const int32_t* pairs, int* n_pairs, std::string* err) {
    const int rc = check_n_windows(n_windows, max_windows, err);
    if (rc != RMX_OK) return rc;
    const int all_pairs = n_buoys * (n_buoys - 1) / 2;
    if (!pairs) {
        if (*n_pairs != 0 && *n_pairs != all_pairs) return refuse(err, "pairs == NULL needs n_pairs == 0 or %d, got %d", all_pairs, *n_pairs);
        *n_pairs = all_pairs;
    }
    if (*n_pairs < 0) return refuse(err, "n_pairs %d < 0", *n_pairs);
    return RMX_OK;
}

// rmx_xcorr_batch_weighted's checks: the weighting, the window count and the bands -- one per window or one for all; a
// banded entry: n_bands of them -- converted to signed bins in r->bins.  n_bands > 1 puts the full band in front (PHAT
// whitens every bin, the band set masks the product).
inline int check_bands(const RequestArgs& a, Request* r, std::string* err) {
    if (a.weighting != RMX_WEIGHT_NONE && a.weighting != RMX_WEIGHT_PHAT)
        return refuse(err, "unknown weighting %u (RMX_WEIGHT_NONE = 0, RMX_WEIGHT_PHAT = 1)", a.weighting);
    const int rc = check_n_windows(a.n_windows, a.max_windows, err);
    if (rc != RMX_OK) return rc;
    const int N = a.n_samples;
    const long M = a.banded ? a.n_bands : 1;
    const long rows = (a.band_cps && a.band_per_window ? (long)a.n_windows : 1L) * M;
    const size_t head = M > 1 ? 2 : 0;
    r->bins.resize(head + (size_t)(2 * rows));
    if (head) {
        r->bins[0] = -N;
        r->bins[1] = N - 1;
    }
    bool all_full = true;
    for (long k = 0; k < rows; ++k) {
        const double lo = a.band_cps ? a.band_cps[2 * k] : -0.5, hi = a.band_cps ? a.band_cps[2 * k + 1] : 0.5;
        int32_t* s = r->bins.data() + head + 2 * k;
        const BandCheck bc = band_to_bins(lo, hi, N, &s[0], &s[1]);
        if (bc != kBandOk) {
            char who[96];
            if (a.banded)
                std::snprintf(who, sizeof who, "band %ld of window %ld%s", k % M, k / M,
                              a.band_per_window ? "" : " (one band set shared by every window)");
            else
                std::snprintf(who, sizeof who, "band of window %ld%s", k, a.band_per_window ? "" : " (one band shared by every window)");
            if (bc == kBandNoInterval) return refuse(err, "%s: [%g, %g] is not an interval inside [-0.5, 0.5] cycles per sample", who, lo, hi);
            return refuse(err, "%s: [%g, %g] keeps no bin of the %ld-point transform", who, lo, hi, 2L * N);
        }
        all_full = all_full && s[0] == -N && s[1] == N - 1;
    }
    r->n_bands = (int)M;
    r->band_per_window = a.band_cps && a.band_per_window;
    r->phat = a.weighting == RMX_WEIGHT_PHAT;
    r->weighted = M > 1 || !(all_full && a.weighting == RMX_WEIGHT_NONE);
    return RMX_OK;
}

// rmx_xcorr_batch_bounded's checks: one interval per pair (r->n_pairs of them), shared or per window -- per GROUP of
// `integrate` windows in an integrated call.  Every interval the full one and nothing integrated is the unbounded call,
// whatever route it takes (the whole-window generic kernels, which a bounded call avoids, included).
inline int check_bounds(const RequestArgs& a, int integrate, Request* r, std::string* err) {
    const int nm1 = a.n_samples - 1, P = r->n_pairs;
    r->bounds = a.lag_bounds;
    r->bounds_per_window = a.bounds_per_window != 0;
    r->bound_rows = r->bounds_per_window ? (long)(a.n_windows / integrate) * P : (long)P;
    bool all_full = true;
    for (long k = 0; k < r->bound_rows; ++k) {
        const int lo = a.lag_bounds[2 * k], hi = a.lag_bounds[2 * k + 1];
        bool full = false;
        if (!lag_interval_ok(lo, hi, a.n_samples, &full))
            return refuse(err, "lag_bounds of %s %ld, pair %ld: [%d, %d] is not an interval inside [%d, %d]",
                          integrate > 1 ? "group" : "window", r->bounds_per_window ? k / P : -1L, k % P, lo, hi, -nm1, nm1);
        all_full = all_full && full;
    }
    r->bounded = !(all_full && integrate == 1);
    return RMX_OK;
}

// An output that a kernel writes while it reads the others (quality, dop_frac) needs a buffer of its own: does
// [p, p + bytes) lie over one of the n arrays of out_bytes each?  `needs` ends the text.
struct OutArray {
    const char* name;
    const void* p;
};
inline int check_overlap(const char* name, const void* p, size_t bytes, const OutArray* outs, int n, size_t out_bytes, const char* needs,
                         std::string* err) {
    const char *q0 = static_cast<const char*>(p), *q1 = q0 + bytes;
    // The array that holds p's first byte is named in front of any other: quality is four times as long as an output, so
    // a quality pointer set ON peak also runs over whatever array the caller's allocator happened to place behind peak,
    // and the text must not depend on that.
    for (int k = 0; k < n; ++k) {
        const char* p0 = static_cast<const char*>(outs[k].p);
        if (p0 <= q0 && q0 < p0 + out_bytes) return refuse(err, "%s overlaps %s: %s", name, outs[k].name, needs);
    }
    for (int k = 0; k < n; ++k) {
        const char* p0 = static_cast<const char*>(outs[k].p);
        if (p0 < q1 && q0 < p0 + out_bytes) return refuse(err, "%s overlaps %s: %s", name, outs[k].name, needs);
    }
    return RMX_OK;
}

// The kernels read a device `iq` and write device outputs through the caller's own pointers, one element per access: a
// complex64 sample (8 bytes), a uint8 I,Q pair (2 bytes: uchar2 indexing and 16-bit buffer loads), a 4-byte output.  A
// device pointer aligned to less than its element is refused, the text naming the array; host pointers only pass
// through the library's own copies and need nothing.  `outs`: the n output arrays, a NULL one (no quality) skipped.
inline int check_alignment(unsigned flags, const void* iq, const OutArray* outs, int n, std::string* err) {
    if (flags & RMX_IN_DEVICE) {
        const bool u8 = (flags & RMX_IN_U8) != 0;
        const unsigned need = u8 ? 2u : 8u, past = (unsigned)(reinterpret_cast<uintptr_t>(iq) % need);
        if (past)
            return refuse(err, "iq is a device pointer %u bytes past a multiple of %u: %s", past, need,
                          u8 ? "uint8 input must be aligned to 2 bytes (one I,Q pair)" : "complex64 input must be aligned to 8 bytes (one sample)");
    }
    if (flags & RMX_OUT_DEVICE)
        for (int k = 0; k < n; ++k) {
            const unsigned past = (unsigned)(reinterpret_cast<uintptr_t>(outs[k].p) % 4u);
            if (outs[k].p && past)
                return refuse(err, "%s is a device pointer %u bytes past a multiple of 4: an output must be aligned to 4 bytes (one element)",
                              outs[k].name, past);
        }
    return RMX_OK;
}

// K and the group count of the grouped entries (integrate, rmx_caf_batch_integrated): the text carries the values
inline int check_groups(int integrate, int n_windows, std::string* err) {
    if (integrate < 1) return refuse(err, "integrate = %d: at least one window per group", integrate);
    if (n_windows <= 0 || n_windows % integrate != 0)
        return refuse(err, "n_windows = %d is not a positive multiple of integrate = %d", n_windows, integrate);
    return RMX_OK;
}

// What check_request and check_caf_request share behind their bounds: refine with its value; quality over one of the n
// other outputs of `slots` elements each (k_quality reads them while it writes quality); the full interval per pair, one
// row for every group, which an integrated call without bounds carries (the integrating kernels always take bounds).
inline int check_refine(int refine, std::string* err) {
    if (refine != 0 && refine != 2 && refine != 4 && refine != 8 && refine != 16)
        return refuse(err, "refine = %d: the fine grid is 1 / U samples with U one of 0 (none), 2, 4, 8, 16", refine);
    return RMX_OK;
}
inline int check_quality_overlap(const float* quality, size_t slots, const OutArray* outs, int n, std::string* err) {
    char needs[96];
    std::snprintf(needs, sizeof needs, "the %zu x 4 floats of quality need a buffer of their own", slots);
    return check_overlap("quality", quality, 4 * slots * sizeof(float), outs, n, slots * sizeof(float), needs, err);
}
inline void full_bounds(int n_samples, Request* r) {
    r->own_bounds.resize(2 * (size_t)r->n_pairs);
    for (int q = 0; q < r->n_pairs; ++q) {
        r->own_bounds[2 * q] = -(n_samples - 1);
        r->own_bounds[2 * q + 1] = n_samples - 1;
    }
    r->bounds = r->own_bounds.data();
    r->bound_rows = r->n_pairs;
    r->bounded = true;
}

// a banded call's per-window (per-group) bounds once per VIRTUAL window: row group * n_bands + band holds the group's row
inline void replicate_bounds(const RequestArgs& a, int K, Request* r) {
    const size_t row = 2 * (size_t)r->n_pairs;
    const long out_rows = (long)(a.n_windows / K) * r->n_bands;
    r->own_bounds.resize((size_t)out_rows * row);
    for (long v = 0; v < out_rows; ++v)
        std::memcpy(&r->own_bounds[(size_t)v * row], a.lag_bounds + (size_t)(v / r->n_bands) * row, row * sizeof(int32_t));
    r->bounds = r->own_bounds.data();
    r->bound_rows *= r->n_bands;
}

// Every check of the nine rmx_xcorr_batch* entries, in the order include/rmx.h promises, so an input with several bad
// arguments is refused for the same one whichever entry it came through: the grouped entries' (integrate, the group
// count), a NULL buffer, a device pointer aligned to less than its element, n_bands, the weighted entry's, the batch
// shape, the bounded entry's, refine, quality over another output.  RMX_OK with *r filled (r->empty: nothing to do), or
// RMX_E_INVAL with *err.
inline int check_request(const RequestArgs& a, Request* r, std::string* err) {
    *r = Request{};
    if (a.bounds_required && !a.lag_bounds) return refuse(err, "NULL buffer");
    if (a.grouped) {   // K and the group count
        const int rc_g = check_groups(a.integrate, a.n_windows, err);
        if (rc_g != RMX_OK) return rc_g;
        // (the full intervals an integrated call without bounds carries are sized by the pair count, so that is looked at here)
        if (a.integrate > 1 && !a.lag_bounds && a.pairs && a.n_pairs < 0) return refuse(err, "n_pairs %d < 0", a.n_pairs);
    }
    const int K = a.grouped ? a.integrate : 1;
    if (!a.iq || !a.lag_int || !a.lag_frac || !a.peak || (a.banded && !a.band_cps)) return refuse(err, "NULL buffer");
    int rc;
    {
        const OutArray outs[4] = {{"lag_int", a.lag_int}, {"lag_frac", a.lag_frac}, {"peak", a.peak}, {"quality", a.quality}};
        rc = check_alignment(a.flags, a.iq, outs, 4, err);
        if (rc != RMX_OK) return rc;
    }
    if (a.banded && (a.n_bands < 1 || a.n_bands > 64)) return refuse(err, "n_bands %d not in 1..64", a.n_bands);
    if (a.banded || a.band_cps || a.weighting != RMX_WEIGHT_NONE) {
        rc = check_bands(a, r, err);
        if (rc != RMX_OK) return rc;
        // (the weighted entry does not look at the pairs of an empty batch)
        if (r->weighted && a.n_windows == 0) {
            r->empty = true;
            return RMX_OK;
        }
    }
    r->n_pairs = a.n_pairs;
    rc = check_batch(a.n_buoys, a.max_windows, a.n_windows, a.pairs, &r->n_pairs, err);
    if (rc != RMX_OK) return rc;
    if (a.n_windows == 0 || r->n_pairs == 0) {
        r->empty = true;
        return RMX_OK;
    }
    if (a.lag_bounds) {
        rc = check_bounds(a, K, r, err);
        if (rc != RMX_OK) return rc;
    }
    rc = check_refine(a.refine, err);
    if (rc != RMX_OK) return rc;
    if (a.quality) {
        const OutArray outs[3] = {{"lag_int", a.lag_int}, {"lag_frac", a.lag_frac}, {"peak", a.peak}};
        rc = check_quality_overlap(a.quality, (size_t)(a.n_windows / K) * r->n_bands * r->n_pairs, outs, 3, err);
        if (rc != RMX_OK) return rc;
    }
    r->integ = K;
    r->refine = a.refine;
    if (K > 1 && !a.lag_bounds) full_bounds(a.n_samples, r);
    // the bounds are per (window, pair) -- per (group, pair) of an integrated call -- and shared by the bands: per-window
    // bounds go to the device once per VIRTUAL window (window-major; per row group * n_bands + band, group-major), so the
    // bounded kernels index them with the virtual window (the row) as they index their outputs.  (The full intervals made
    // above are the shared form, one row for every group and band: nothing to replicate.)
    if (r->n_bands > 1 && r->bounded && r->bounds_per_window) replicate_bounds(a, K, r);
    return RMX_OK;
}

// The tail of a Doppler call's check, behind its head (below): `a` with n_pairs resolved; the weighted entry's checks, the
// bounded entry's, dop_frac over another output, refine, quality over one of the five other outputs (k_quality reads
// peak and dop_idx while it writes quality), a device quality aligned to less than its element.  The bands stay per
// window, the bounds are per GROUP and every output extent is G * n_pairs slots, G = n_windows / K; K > 1 without bounds
// carries the full interval per pair, as check_request's.  The banded search (rmx_caf_batch_bands, a.banded): n_bands band
// rows per window, every extent n_windows * n_bands * n_pairs slots, and per-window bounds replicated per virtual window
// as check_request replicates them.
inline int check_caf_request(const RequestArgs& a, const int32_t* dop_idx, const float* dop_frac, Request* r, std::string* err) {
    *r = Request{};
    r->n_pairs = a.n_pairs;
    const int K = a.grouped ? a.integrate : 1;
    const size_t slots = (size_t)(a.n_windows / K) * (size_t)(a.banded ? a.n_bands : 1) * a.n_pairs;
    const OutArray outs[5] = {{"dop_idx", dop_idx}, {"lag_int", a.lag_int}, {"lag_frac", a.lag_frac}, {"peak", a.peak}, {"dop_frac", dop_frac}};
    int rc;
    if (a.banded || a.band_cps || a.weighting != RMX_WEIGHT_NONE) {
        rc = check_bands(a, r, err);
        if (rc != RMX_OK) return rc;
    }
    if (a.lag_bounds) {
        rc = check_bounds(a, K, r, err);
        if (rc != RMX_OK) return rc;
    }
    if (dop_frac) {
        char needs[96];
        std::snprintf(needs, sizeof needs, "its %zu floats need a buffer of their own", slots);
        rc = check_overlap("dop_frac", dop_frac, slots * sizeof(float), outs, 4, slots * sizeof(float), needs, err);
        if (rc != RMX_OK) return rc;
    }
    rc = check_refine(a.refine, err);
    if (rc != RMX_OK) return rc;
    if (a.quality) {
        rc = check_quality_overlap(a.quality, slots, outs, dop_frac ? 5 : 4, err);
        if (rc != RMX_OK) return rc;
        const OutArray q[1] = {{"quality", a.quality}};
        rc = check_alignment(a.flags & RMX_OUT_DEVICE, nullptr, q, 1, err);
        if (rc != RMX_OK) return rc;
    }
    r->integ = K;
    r->refine = a.refine;
    if (K > 1 && !a.lag_bounds) full_bounds(a.n_samples, r);
    if (r->n_bands > 1 && r->bounded && r->bounds_per_window) replicate_bounds(a, K, r);
    return RMX_OK;
}

// Every check of the five rmx_caf_batch* entries, in the order include/rmx.h promises, as check_request is every check of
// a correlation call.  The head: a NULL buffer (rmx_caf_batch_bands: band_cps too), a device pointer aligned to less than
// its element (the five arrays), n_dopplers, n_bands (rmx_caf_batch_bands), the group count (a.grouped with
// a.integrate != 1 only: one window per group takes an empty batch), the batch shape, the empty batch, the pair list; then
// the tail above on the resolved pair count.  RMX_OK with *r filled
// (r->empty: nothing to do), or RMX_E_INVAL with *err.
inline int check_caf_request(const RequestArgs& a, Request* r, std::string* err) {
    *r = Request{};
    if (!a.iq || !a.dop_idx || !a.lag_int || !a.lag_frac || !a.peak || !a.doppler_cps || (a.banded && !a.band_cps))
        return refuse(err, "NULL buffer");
    const OutArray outs[5] = {{"dop_idx", a.dop_idx}, {"dop_frac", a.dop_frac}, {"lag_int", a.lag_int}, {"lag_frac", a.lag_frac}, {"peak", a.peak}};
    int rc = check_alignment(a.flags, a.iq, outs, 5, err);
    if (rc != RMX_OK) return rc;
    if (a.n_dopplers < 1 || a.n_dopplers > 4096) return refuse(err, "n_dopplers %d not in 1..4096", a.n_dopplers);
    if (a.banded && (a.n_bands < 1 || a.n_bands > 64)) return refuse(err, "n_bands %d not in 1..64", a.n_bands);
    if (a.grouped && a.integrate != 1) {
        rc = check_groups(a.integrate, a.n_windows, err);
        if (rc != RMX_OK) return rc;
    }
    RequestArgs resolved = a;
    rc = check_batch(a.n_buoys, a.max_windows, a.n_windows, a.pairs, &resolved.n_pairs, err);
    if (rc != RMX_OK) return rc;
    if (a.n_windows == 0 || resolved.n_pairs == 0) {
        r->n_pairs = resolved.n_pairs;
        r->empty = true;
        return RMX_OK;
    }
    if (check_pair_list(a.n_buoys, a.pairs, resolved.n_pairs, err) != 0) return RMX_E_INVAL;
    return check_caf_request(resolved, a.dop_idx, a.dop_frac, r, err);
}

}  // namespace host
}  // namespace rmx
