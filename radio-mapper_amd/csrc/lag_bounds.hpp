// lag_bounds.hpp -- the caller-given lag window of rmx_xcorr_batch_bounded (include/rmx.h).
//
// Every peak-searching kernel has a bounded instantiation next to the unbounded one.  The bounded one reads, per
// (window w, pair q), the interval [lo, hi] in lag units at b + w * wstride + 2 q (wstride = 0: one interval per pair,
// shared by all windows) and works in 'full' indices klo = lo + N - 1, khi = hi + N - 1:
//   - every |r|^2 outside [klo, khi] becomes the -1 sentinel the kernels already use for the excluded lag -N, before the
//     lane, wave and workgroup maximum (every in-window value is >= +0, so an all-zero window resolves to klo);
//   - the resolver sets frac = 0 when k* is klo or khi (the slice's edges).  The neighbour taps of an interior k* lie
//     inside the interval, so they are never masked and the halo logic does not change.
// The unbounded kernels take no bounds argument at all: the kernels carry them as a trailing template pack (empty for
// the unbounded instantiation, so its argument list and its code are the library's as before).
#pragma once

#include <hip/hip_runtime.h>

namespace rmx {

struct LagBounds {
    const int* b;    // device int32 [.][n_pairs][2]
    long wstride;    // int32 elements per window: 2 n_pairs, or 0 for the shared form
    long w0;         // kernels that index (window-in-chunk * n_pairs + pair) slots: global index of the chunk's window 0
    int n_pairs;     // ... and the pairs per window
};

// the LagBounds of a kernel's trailing pack: its first member (integrate.hpp adds a second), or none
__device__ __forceinline__ LagBounds lag_bounds_of() { return LagBounds{nullptr, 0, 0, 0}; }
template <class... More>
__device__ __forceinline__ LagBounds lag_bounds_of(LagBounds lb, More...) { return lb; }

// 'full' index interval of window w (global index), pair q (output index); nm1 = N - 1
__device__ __forceinline__ void lag_window(const LagBounds& lb, long w, int q, int nm1, int& klo, int& khi) {
    const int* p = lb.b + w * lb.wstride + 2 * q;
    klo = p[0] + nm1;
    khi = p[1] + nm1;
}

// the same for slot = window-in-chunk * n_pairs + pair
__device__ __forceinline__ void lag_window_slot(const LagBounds& lb, long slot, int nm1, int& klo, int& khi) {
    lag_window(lb, lb.w0 + slot / lb.n_pairs, (int)(slot % lb.n_pairs), nm1, klo, khi);
}

// |r|^2 at 'full' index k, or the -1 sentinel outside [klo, khi] (one subtract, one unsigned compare, one select)
__device__ __forceinline__ float lag_mask(float m, int k, int klo, int khi) {
    return (unsigned)(k - klo) <= (unsigned)(khi - klo) ? m : -1.0f;
}

}  // namespace rmx
