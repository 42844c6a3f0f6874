// caf_select.hpp -- the Doppler search's selection kernels (rmx_caf_batch): the best hypothesis per pair-window, as a
// running maximum behind every hypothesis (k_caf_select) or over all hypotheses of one launch (k_caf_select_all).
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

}  // namespace rmx
