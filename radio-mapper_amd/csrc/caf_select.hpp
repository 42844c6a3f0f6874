// caf_select.hpp -- the Doppler search's selection kernels (rmx_caf_batch): the best hypothesis per pair-window, as a
// running maximum behind every hypothesis (k_caf_select) or over all hypotheses of one launch (k_caf_select_all).
// The _fd kernels (rmx_caf_batch_request with dop_frac) make the same selection and add the sub-grid Doppler estimate:
// the S5 parabola through the winner's peak and its two neighbour hypotheses' peaks, in grid indices.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace rmx {

// The tail of k_refine's and k_quality's parameter pack under rmx_caf_batch_quality (refine.hpp, quality.hpp): output slot
// o = (window, pair) correlates operand i from the kernel's own spectra (the un-rotated set) at (window, i) and operand j
// from the de-rotated set of ITS winner dop[o] -- chosen by the selection kernels below, which have run.
// rmx_caf_batch_integrated: a slot is a (group, pair) and the kernels walk the group's a.k windows, window g K + kw of
// either set; dop is indexed by the group's slot and hyp_items stays W * B, so virtual window dop[o] * W + g K + kw.
//   every hypothesis resident (the one-launch path of N = 4096): d < 0; the set of hypothesis h starts hyp_items items
//       into spec_j, and slot o reads item dop[o] * hyp_items + window * n_buoys + j (virtual window dop[o] * W + window);
//   one hypothesis resident (the second sweep of the per-hypothesis routes): d >= 0 is the hypothesis whose de-rotated
//       set spec_j holds, laid out as the kernel's own; a workgroup whose slot was won by another hypothesis returns at
//       once, in front of its first barrier, and touches nothing.
struct CafWinner {
    const int* dop;          // device dop_idx, [n_windows][n_pairs] ([G][n_pairs] integrated): indexed by the global output slot
    const float2* spec_j;    // the de-rotated spectra, [item][L] in the layout's order
    long hyp_items;          // items (window, buoy) per resident hypothesis, or 0
    int d;                   // the one resident hypothesis, or -1: all are
};

template <class... P>
struct caf_pack : std::false_type {};
template <>
struct caf_pack<CafWinner> : std::true_type {};
template <class... P>
inline constexpr bool kCafWinner = caf_pack<P...>::value;
__device__ __forceinline__ CafWinner caf_winner_of(CafWinner cw) { return cw; }

// ---- CAF helper: running best hypothesis per pair-window -------------------------------------------
__global__ void k_caf_select(int d, long first, long n, const int* __restrict__ lag_d, const float* __restrict__ frac_d,
                             const float* __restrict__ peak_d, int* __restrict__ dop, int* __restrict__ lag,
                             float* __restrict__ frac, float* __restrict__ peak) {
    const long i = first + (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= first + n) return;
    if (d == 0 || peak_d[i] > peak[i]) {   // strict: ties keep the lowest d
        dop[i] = d; lag[i] = lag_d[i]; frac[i] = frac_d[i]; peak[i] = peak_d[i];
    }
}


// the same over all hypotheses of one launch: arrays [n_dop][n], d-major first maximum (strict >: ties keep the lowest d)
__global__ void k_caf_select_all(int n_dop, long n, const int* __restrict__ lag_d, const float* __restrict__ frac_d,
                                 const float* __restrict__ peak_d, int* __restrict__ dop, int* __restrict__ lag,
                                 float* __restrict__ frac, float* __restrict__ peak) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int bd = 0;
    float bp = peak_d[i];
    for (int d = 1; d < n_dop; ++d) {
        const float pd = peak_d[(long)d * n + i];
        if (pd > bp) { bp = pd; bd = d; }
    }
    dop[i] = bd; lag[i] = lag_d[(long)bd * n + i]; frac[i] = frac_d[(long)bd * n + i]; peak[i] = bp;
}

// dop_frac of a winner d* with neighbour peaks a (d* - 1) and c (d* + 1) around b: (a - c) / (2 (a - 2 b + c)) in double
// from the float32 peaks.  The first-maximum rule gives a < b and c <= b, so the denominator is negative.
__device__ __forceinline__ float caf_dop_frac(float a, float b, float c) {
    const double den = 2.0 * ((double)a - 2.0 * (double)b + (double)c);
    return den == 0.0 ? 0.0f : (float)(((double)a - (double)c) / den);
}

// k_caf_select with dop_frac.  The three taps are not all known when hypothesis d wins, so each slot keeps three floats
// in nb (ctx scratch, [3][n_all]: the previous hypothesis' peak, the winner's left and right neighbour) and the kernel
// behind the last hypothesis (d == n_dop - 1) resolves dop_frac.  The four other outputs are written exactly as
// k_caf_select writes them.
__global__ void k_caf_select_fd(int d, int n_dop, long first, long n, long n_all, const int* __restrict__ lag_d,
                                const float* __restrict__ frac_d, const float* __restrict__ peak_d, int* __restrict__ dop,
                                int* __restrict__ lag, float* __restrict__ frac, float* __restrict__ peak,
                                float* __restrict__ nb, float* __restrict__ dop_frac) {
    const long i = first + (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= first + n) return;
    float* prev = nb + i;
    float* left = nb + n_all + i;
    float* right = nb + 2 * n_all + i;
    const float pd = peak_d[i];
    if (d == 0 || pd > peak[i]) {   // strict: ties keep the lowest d
        dop[i] = d; lag[i] = lag_d[i]; frac[i] = frac_d[i]; peak[i] = pd;
        *left = d == 0 ? 0.0f : *prev;
        *right = 0.0f;
    } else if (dop[i] == d - 1) {
        *right = pd;
    }
    *prev = pd;
    if (d == n_dop - 1) {
        const int bd = dop[i];
        dop_frac[i] = (bd == 0 || bd == n_dop - 1) ? 0.0f : caf_dop_frac(*left, peak[i], *right);
    }
}

// k_caf_select_all with dop_frac: all peaks of a slot are in peak_d
__global__ void k_caf_select_all_fd(int n_dop, long n, const int* __restrict__ lag_d, const float* __restrict__ frac_d,
                                    const float* __restrict__ peak_d, int* __restrict__ dop, int* __restrict__ lag,
                                    float* __restrict__ frac, float* __restrict__ peak, float* __restrict__ dop_frac) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int bd = 0;
    float bp = peak_d[i];
    for (int d = 1; d < n_dop; ++d) {
        const float pd = peak_d[(long)d * n + i];
        if (pd > bp) { bp = pd; bd = d; }
    }
    dop[i] = bd; lag[i] = lag_d[(long)bd * n + i]; frac[i] = frac_d[(long)bd * n + i]; peak[i] = bp;
    dop_frac[i] = (bd == 0 || bd == n_dop - 1) ? 0.0f
                                               : caf_dop_frac(peak_d[(long)(bd - 1) * n + i], bp, peak_d[(long)(bd + 1) * n + i]);
}

}  // namespace rmx
