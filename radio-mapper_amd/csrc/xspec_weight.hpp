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

// ---- where each per-transform forward kernel stores natural bin k of its L-point spectrum ---------------------------
// (the weighted store epilogues and k_refine, refine.hpp, which walks the stored spectra in storage order, share these)
// k_fwd, role C (fft_r16.hpp): spec[item][j][t] float4 = slots (2 j, 2 j + 1) of thread t; with p = t & 1 and
// u = t >> 1 = 16 k0 + k1, slot s = k2 holds natural bin 2 (k0 + 16 k1 + 256 s) + p = xbin_kfwd(p, u) + kXbinKfwdSlot * s
// (k_fwd expands the expression in place: through an inlined function hipcc allocated the weighted k_fwd's registers and
// ordered its address arithmetic differently -- the same instructions otherwise --, and tools/isa_diff.py holds the existing
// kernels to their bodies; xbin_kfwd is the same expansion for every other caller)
constexpr int kXbinKfwdSlot = 512;
#define RMX_XBIN_KFWD(p, u) (2 * (((u) >> 4) + 16 * ((u) & 15)) + (p))
__device__ __forceinline__ int xbin_kfwd(int p, int u) { return RMX_XBIN_KFWD(p, u); }
// g_fwd_small: spec[item][n], position n holds natural bin bitrev(n) (the DIF order of the LDS transform)
__device__ __forceinline__ int xbin_small(int n, int logL) { return (int)(__brev((unsigned)n) >> (32 - logL)); }
// forward g_rows (four-step): spec[item][row][n] holds natural bin k1 + L1 k2, k1 = bitrev(row index) over row_bits,
// k2 = bitrev(n) over logR (the column pass's and the row pass's DIF orders)
__device__ __forceinline__ int xbin_rows_k1(int row, int row_bits) { return (int)(__brev((unsigned)row) >> (32 - row_bits)); }
__device__ __forceinline__ int xbin_rows(int k1, int n, int row_bits, int logR) {
    return k1 + ((int)(__brev((unsigned)n) >> (32 - logR)) << row_bits);
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
