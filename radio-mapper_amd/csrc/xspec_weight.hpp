// xspec_weight.hpp -- the cross-spectrum weighting of rmx_xcorr_batch_weighted (include/rmx.h): a band mask and PHAT.
//
// Both weights factor per buoy -- M X_j conj(M X_i) = M X_j conj(X_i) for a 0/1 mask M, and
// X_j conj(X_i) / (|X_i| |X_j|) = (X_j / |X_j|) conj(X_i / |X_i|) -- so they are applied where each forward spectrum is
// stored, and every pair kernel, inverse transform and peak search runs unchanged on the weighted spectra.
// Each per-transform forward kernel (k_fwd, g_fwd_small, the forward g_rows) has a weighted instantiation next to the
// plain one: the weight is a trailing template pack, empty for the plain instantiation (so its argument list and its
// code are the library's as before), one XWeight for the weighted one.  Per stored bin the epilogue maps the stored
// position to the natural bin k of the L-point transform (each kernel has its own order), keeps the bin when its signed
// index s (s = k, or k - L for k >= N) lies in the window's [s_lo, s_hi] -- one subtract, one mask, one unsigned
// compare -- and with PHAT scales it to magnitude `unit`, the power-of-two forward scale every stored spectrum of that
// kernel carries (one v_rsq_f32, three multiplies; a zero bin stays zero, so a dead receiver gives zeros, never NaN).
#pragma once

#include <hip/hip_runtime.h>

namespace rmx {

struct XWeight {
    const int* band;   // device int32 [.][2] = signed bins [s_lo, s_hi] kept, -N <= s_lo <= s_hi <= N - 1
    long wstride;      // int32 elements per window: 2, or 0 for one band shared by every window
    long w0;           // kernels that index chunk-local items: global index of the launch's window 0
    int n_buoys;       // items (transforms) per window
    int phat;          // 1: every kept bin scaled to magnitude `unit`
    float unit;        // the forward scale of the kernel's stored spectra (what a bin of magnitude 1 is stored as)
};

template <class... WT>
__device__ __forceinline__ XWeight xweight_of(WT... wt) {
    if constexpr (sizeof...(WT) > 0) {
        return XWeight(wt...);
    } else {
        return XWeight{nullptr, 0, 0, 0, 0, 0.0f};
    }
}

// the kept set of one window as a test on the natural bin k: (k - s_lo) mod L <= s_hi - s_lo
struct XBand {
    int lo;         // s_lo
    unsigned span;  // s_hi - s_lo
};
__device__ __forceinline__ XBand xband_of(const XWeight& wt, long w) {
    const int* p = wt.band + w * wt.wstride;
    return XBand{p[0], (unsigned)(p[1] - p[0])};
}

// the stored value v of natural bin k (lmask = L - 1) after weighting
__device__ __forceinline__ float2 xweight_apply(const XWeight& wt, const XBand& bd, int k, int lmask, float2 v) {
    if (wt.phat) {
        const float m2 = v.x * v.x + v.y * v.y;
        const float r = m2 > 0.0f ? __builtin_amdgcn_rsqf(m2) * wt.unit : 0.0f;
        v = make_float2(v.x * r, v.y * r);
    }
    const bool keep = (unsigned)((k - bd.lo) & lmask) <= bd.span;
    return keep ? v : make_float2(0.0f, 0.0f);
}

}  // namespace rmx
