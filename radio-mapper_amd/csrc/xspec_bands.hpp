// xspec_bands.hpp -- several bands per window over ONE set of forward spectra, rmx_xcorr_batch_bands (include/rmx.h).
//
// A band is a 0/1 weight, M X_j conj(M X_i) = M (X_j conj(X_i)), so the mask can sit where the product is formed instead
// of where each spectrum is stored (xspec_weight.hpp).  The forward kernels then run once per (window, buoy), unmasked --
// the plain instantiations, or under PHAT the weighted ones with the full band --, and every kernel that forms the product
// has a banded instantiation: the trailing template pack that is empty for the plain kernel and one LagBounds for the
// bounded one is <BandSet> or <LagBounds, BandSet> here.  The empty pack leaves the kernel's argument list and code as
// they are.
//   k_pair_res, k_pair_str (pair4096.hpp)   a thread's 16 product slots are the same 16 bins for every pair of the
//                                           workgroup: a 16-bit keep word per thread, built once, zeroes the product
//   g_pair_small, inverse g_rows            the product is formed bin by bin on load: a dropped bin loads nothing and is
//   (generic_path.hpp)                      stored as +0
// A work item's window index v is VIRTUAL, window-major: real window v / n_bands (both operands' spectra), band
// v % n_bands, output row v.  The host hands the lag windows over per virtual window (a real window's interval repeated
// for each of its bands), so the bounded code of a kernel indexes them with v as it indexes everything else.
// A dropped bin is exactly +0, which is what the product of two masked spectra is, and a kept bin is the product of the
// same two stored values: slot (w, m, q) carries the bits of the weighted call with band[w][m].
//
// The Doppler search under several bands (rmx_caf_batch_bands): the same banded pair kernels with operand j from the
// de-rotated set.  Per hypothesis nothing changes.  With every hypothesis in ONE launch of N = 4096 the virtual window is
// v = (d W + w) n_bands + m and the kernels get i_wrap = W n_bands: operand j at window v / n_bands of the de-rotated set,
// operand i, the band and the lag interval those of virtual window v mod i_wrap, the output row v.  i_wrap = 0 is the
// correlation above.
//
// Banded AND integrated (rmx_xcorr_batch_bands_integrated): the third pack, <LagBounds, Integrate, BandSet>, on the
// integrating pair kernels (integrate.hpp) and on k_refine / k_quality.  A work item is an output ROW r = g n_bands + m
// -- group g, band m -- and a pair: it walks the real windows g K ... g K + K - 1 of the chunk, masks each window's
// product with band (window, m) -- looked up per WINDOW: the windows of a group may carry different bands in column m --
// and adds |r|^2 in window order into the accumulators of the integrating kernel.  The lag interval and the outputs are
// row r's.  A skipped +0 here is a stored +0 in the single-band integrated call with band[.][m], and the K terms of a lag
// are added by one thread in window order on both sides: slot (g, m, q) carries that call's bits.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "integrate.hpp"
#include "lag_bounds.hpp"
#include "xspec_weight.hpp"

namespace rmx {

struct BandSet {
    const int* bins;   // device int32 [.][n_bands][2] = signed bins [s_lo, s_hi] kept, -N <= s_lo <= s_hi <= N - 1
    long wstride;      // int32 elements per real window: 2 n_bands, or 0 for one set shared by every window
    long w0;           // global index of the real window that virtual window 0 of the launch belongs to
    int n_bands;       // bands per window, >= 1
};

template <class... P>
struct band_pack : std::false_type {};
template <>
struct band_pack<BandSet> : std::true_type {};
template <>
struct band_pack<LagBounds, BandSet> : std::true_type {};
template <>
struct band_pack<LagBounds, Integrate, BandSet> : std::true_type {};
template <class... P>
inline constexpr bool kBanded = band_pack<P...>::value;

// the banded integrating pack is an integrating pack (integrate.hpp)
template <>
struct integ_pack<LagBounds, Integrate, BandSet> : std::true_type {};
__device__ __forceinline__ LagBounds integ_bounds(LagBounds lb, Integrate, BandSet) { return lb; }
__device__ __forceinline__ int integ_windows(LagBounds, Integrate ig, BandSet) { return ig.k; }

// does the pack start with a LagBounds (the bounded, the integrating and the bounded banded instantiations)?
template <class... P>
struct bounds_pack : std::false_type {};
template <class... More>
struct bounds_pack<LagBounds, More...> : std::true_type {};
template <class... P>
inline constexpr bool kHasBounds = bounds_pack<P...>::value;

__device__ __forceinline__ LagBounds lag_bounds_of(BandSet) { return LagBounds{nullptr, 0, 0, 0}; }
__device__ __forceinline__ BandSet band_set_of(BandSet bs) { return bs; }
__device__ __forceinline__ BandSet band_set_of(LagBounds, BandSet bs) { return bs; }
__device__ __forceinline__ BandSet band_set_of(LagBounds, Integrate, BandSet bs) { return bs; }
// bands per window of an integrating pack: the row stride of its work items (1 without a band set)
__device__ __forceinline__ int integ_bands(LagBounds, Integrate) { return 1; }
__device__ __forceinline__ int integ_bands(LagBounds, Integrate, BandSet bs) { return bs.n_bands; }

// virtual window v of the launch -> the real window (chunk-local) whose spectra it correlates / its band
__device__ __forceinline__ int band_real_window(const BandSet& bs, int v) { return v / bs.n_bands; }
__device__ __forceinline__ XBand band_of_virtual(const BandSet& bs, int v) {
    const int wr = v / bs.n_bands, m = v - wr * bs.n_bands;
    const int* p = bs.bins + (bs.w0 + wr) * bs.wstride + 2 * m;
    return XBand{p[0], (unsigned)(p[1] - p[0])};
}

// banded integrating kernels: band m of real window wr (chunk-local) -- per window, whatever the group
__device__ __forceinline__ XBand band_of_window(const BandSet& bs, long wr, int m) {
    const int* p = bs.bins + (bs.w0 + wr) * bs.wstride + 2 * m;
    return XBand{p[0], (unsigned)(p[1] - p[0])};
}

// xweight_apply's test: is natural bin k (lmask = L - 1) inside the band?
__device__ __forceinline__ bool xband_keeps(const XBand& bd, int k, int lmask) { return (unsigned)((k - bd.lo) & lmask) <= bd.span; }

}  // namespace rmx
