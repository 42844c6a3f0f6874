// caf_select.hpp -- the Doppler search's selection kernels (rmx_caf_batch): the best hypothesis per pair-window, as a
// running maximum behind every hypothesis (k_caf_select) or over all hypotheses of one launch (k_caf_select_all).
// The _fd kernels (rmx_caf_batch_request with dop_frac) make the same selection and add the sub-grid Doppler estimate:
// the S5 parabola through the winner's peak and its two neighbour hypotheses' peaks, in grid indices.
#pragma once
#include <hip/hip_runtime.h>

namespace rmx {

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
