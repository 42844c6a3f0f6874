// integrate.hpp -- noncoherent integration over consecutive windows, rmx_xcorr_batch_integrated (include/rmx.h).
//
// K consecutive windows form a group; the group's pair (i, j) has ONE peak search, on
//     s[k] = sum over the group's windows, in window order, of |c_w[k]|^2     (float32)
// with the taps m[k] = sqrt(s[k]).  The forward kernels run unchanged on all windows (the spectra scratch holds a chunk
// of whole groups).  Each of the three pair / peak kernels of the per-transform routes has an integrating
// instantiation: the trailing template pack that is empty for the plain kernel and one LagBounds for the bounded one
// is <LagBounds, Integrate> here (an unbounded integrated call passes the full interval, which changes nothing).
// Its work item is (group, pair) instead of (window, pair): it walks the group's K windows, adds every window's |r|^2
// into per-thread registers -- each thread owns the same lags in every window, at most 16 of them, so the order of
// the additions is the window order whatever the scheduling -- and runs the masking, the argmax, the taps and the
// parabola once, on the sums:
//   k_pair_str    (N = 4096)        pair_body_integ, pair4096.hpp: acc[16] beside mag[16]
//   g_pair_small  (L <= small_maxl) pair_small_integ, generic_path.hpp: lag m = tid + e nthr in acc[e]
//   g_cols_inv    (four-step)       cols_inv_integ, generic_path.hpp: a tile is a set of whole columns and the column
//                                   pass is the last one, so the sum is local to the tile; the summed |r|^2 goes back
//                                   into the tile image and the tile record, the halo and g_final run as they are
// The lag windows of an integrating kernel are indexed by GROUP (lag_bounds.hpp: w is the group, wstride the int32
// elements per group).
// The Doppler search may be integrated too (rmx_caf_batch_integrated): the pack <LagBounds, Integrate, CafOperand> below
// gives k_pair_str and g_pair_small their operand j from the de-rotated spectra; the four-step row kernels take that set
// as they are (spec_j) and cols_inv_integ sums whatever products they made.
// A banded call may be integrated too (rmx_xcorr_batch_bands_integrated): xspec_bands.hpp adds the pack
// <LagBounds, Integrate, BandSet>, whose work item is (group, band, pair) and whose lag windows and outputs are indexed by
// the row group * n_bands + band.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "lag_bounds.hpp"

namespace rmx {

struct Integrate {
    int k;   // windows per group, >= 2 (K = 1 is the plain call and never reaches these instantiations)
};

constexpr int kIntegMaxPerThread = 16;   // lags a thread of an integrating kernel accumulates

template <class... P>
struct integ_pack : std::false_type {};
template <>
struct integ_pack<LagBounds, Integrate> : std::true_type {};
template <class... P>
inline constexpr bool kIntegrating = integ_pack<P...>::value;

__device__ __forceinline__ LagBounds integ_bounds(LagBounds lb, Integrate) { return lb; }
__device__ __forceinline__ int integ_windows(LagBounds, Integrate ig) { return ig.k; }

// The integrated Doppler search (rmx_caf_batch_integrated): the pack <LagBounds, Integrate, CafOperand> of k_pair_str and
// g_pair_small reads operand j from the kernel's second spectrum set, spec_j -- the de-rotated spectra -- instead of the
// first.  Where one launch holds every hypothesis (N = 4096) a work item is a VIRTUAL group gv = d * groups + g: its K
// de-rotated windows are virtual windows gv * K + kw of spec_j (d * W + g * K + kw, contiguous), operand i and the lag
// interval are those of the REAL group gv % groups, the output slot stays virtual.  groups == 0: spec_j holds one
// hypothesis, laid out as spec, and the group is the real one.
struct CafOperand {
    int groups;   // real groups per hypothesis of a launch over every hypothesis, or 0
};
template <>
struct integ_pack<LagBounds, Integrate, CafOperand> : std::true_type {};
template <class... P>
struct caf_operand_pack : std::false_type {};
template <>
struct caf_operand_pack<LagBounds, Integrate, CafOperand> : std::true_type {};
template <class... P>
inline constexpr bool kCafOperand = caf_operand_pack<P...>::value;
__device__ __forceinline__ LagBounds integ_bounds(LagBounds lb, Integrate, CafOperand) { return lb; }
__device__ __forceinline__ int integ_windows(LagBounds, Integrate ig, CafOperand) { return ig.k; }
__device__ __forceinline__ int caf_groups(LagBounds, Integrate, CafOperand co) { return co.groups; }

}  // namespace rmx
