// solve_path.hpp -- k_solve, the batched hyperbolic position solve of rmx_solve_batch.
#pragma once
#include <hip/hip_runtime.h>

namespace rmx {

// ---- batched hyperbolic position solve (rmx_solve_batch) --------------------------------------------
// One thread per window: 3 unknowns, P residuals, everything in float64 registers; the buoy table and
// the pair list sit in LDS.  The lag arrays are read transposed-strided (lane = window), which is a
// few hundred bytes per window and iteration: the kernel is latency-bound by its dependent
// sqrt/divide chains, not by memory.
constexpr int kSolveMaxBuoys = 64;
constexpr int kSolveMaxPairs = kSolveMaxBuoys * (kSolveMaxBuoys - 1) / 2;
__global__ __launch_bounds__(64) void k_solve(const double* __restrict__ buoy_xyz, int n_buoys,
                                              const int* __restrict__ pairs, int n_pairs,
                                              const int* __restrict__ lag_int, const float* __restrict__ lag_frac,
                                              const float* __restrict__ weight, double metres_per_sample,
                                              int n_windows, int max_iter, double* __restrict__ pos,
                                              double* __restrict__ cost, int* __restrict__ iters) {
#pragma clang fp contract(off)   // same roundings as the numpy restatement wherever the order is the same
    __shared__ double sb[kSolveMaxBuoys * 3];
    __shared__ short spair[kSolveMaxPairs * 2];
    for (int i = threadIdx.x; i < n_buoys * 3; i += blockDim.x) sb[i] = buoy_xyz[i];
    for (int i = threadIdx.x; i < n_pairs * 2; i += blockDim.x) spair[i] = (short)pairs[i];
    __syncthreads();
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_windows) return;
    const int* li = lag_int + (long)w * n_pairs;
    const float* lf = lag_frac + (long)w * n_pairs;
    const float* wg = weight ? weight + (long)w * n_pairs : nullptr;
    double px = 0, py = 0, pz = 0;
    for (int b = 0; b < n_buoys; ++b) { px += sb[3 * b]; py += sb[3 * b + 1]; pz += sb[3 * b + 2]; }
    px /= n_buoys; py /= n_buoys; pz /= n_buoys;
    auto f_at = [&](double x, double y, double z) -> double {
        double f = 0;
        for (int q = 0; q < n_pairs; ++q) {
            const double* b1 = sb + 3 * spair[2 * q];
            const double* b2 = sb + 3 * spair[2 * q + 1];
            const double n1 = sqrt((x - b1[0]) * (x - b1[0]) + (y - b1[1]) * (y - b1[1]) + (z - b1[2]) * (z - b1[2]));
            const double n2 = sqrt((x - b2[0]) * (x - b2[0]) + (y - b2[1]) * (y - b2[1]) + (z - b2[2]) * (z - b2[2]));
            const double d = ((double)li[q] + (double)lf[q]) * metres_per_sample;
            const double r = n2 - n1 - d;
            f += (wg ? (double)wg[q] : 1.0) * r * r;
        }
        return f;
    };
    double lam = 1e-3;
    double f = f_at(px, py, pz);
    int it = 0;
    while (it < max_iter) {
        ++it;
        double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, g0 = 0, g1 = 0, g2 = 0;
        for (int q = 0; q < n_pairs; ++q) {
            const double* b1 = sb + 3 * spair[2 * q];
            const double* b2 = sb + 3 * spair[2 * q + 1];
            const double v1x = px - b1[0], v1y = py - b1[1], v1z = pz - b1[2];
            const double v2x = px - b2[0], v2y = py - b2[1], v2z = pz - b2[2];
            const double n1 = sqrt(v1x * v1x + v1y * v1y + v1z * v1z);
            const double n2 = sqrt(v2x * v2x + v2y * v2y + v2z * v2z);
            const double d = ((double)li[q] + (double)lf[q]) * metres_per_sample;
            const double r = n2 - n1 - d;
            const double jx = v2x / n2 - v1x / n1, jy = v2y / n2 - v1y / n1, jz = v2z / n2 - v1z / n1;
            const double ww = wg ? (double)wg[q] : 1.0;
            a00 += ww * jx * jx; a01 += ww * jx * jy; a02 += ww * jx * jz;
            a11 += ww * jy * jy; a12 += ww * jy * jz; a22 += ww * jz * jz;
            g0 += ww * jx * r; g1 += ww * jy * r; g2 += ww * jz * r;
        }
        // (A + lam diag A) delta = -g by Cholesky; a failed factorisation counts as a rejected step
        const double d00 = a00 * (1.0 + lam), d11 = a11 * (1.0 + lam), d22 = a22 * (1.0 + lam);
        bool ok = d00 > 0.0;
        const double l00 = sqrt(ok ? d00 : 1.0);
        const double l10 = a01 / l00, l20 = a02 / l00;
        const double t11 = d11 - l10 * l10;
        ok = ok && t11 > 0.0;
        const double l11 = sqrt(ok ? t11 : 1.0);
        const double l21 = (a12 - l20 * l10) / l11;
        const double t22 = d22 - l20 * l20 - l21 * l21;
        ok = ok && t22 > 0.0;
        const double l22 = sqrt(ok ? t22 : 1.0);
        bool accepted = false;
        double dn = 0.0;
        if (ok) {
            const double y0 = -g0 / l00;
            const double y1 = (-g1 - l10 * y0) / l11;
            const double y2 = (-g2 - l20 * y0 - l21 * y1) / l22;
            const double dz = y2 / l22;
            const double dy = (y1 - l21 * dz) / l11;
            const double dx = (y0 - l10 * dy - l20 * dz) / l00;
            const double fn = f_at(px + dx, py + dy, pz + dz);
            if (fn < f) {
                px += dx; py += dy; pz += dz;
                f = fn;
                accepted = true;
                dn = sqrt(dx * dx + dy * dy + dz * dz);
            }
        }
        if (accepted) {
            lam = lam / 3.0 > 1e-12 ? lam / 3.0 : 1e-12;
            if (dn < 1e-4) break;
        } else {
            lam *= 4.0;
            if (lam > 1e12) break;
        }
    }
    pos[3 * (long)w] = px; pos[3 * (long)w + 1] = py; pos[3 * (long)w + 2] = pz;
    cost[w] = f;
    iters[w] = it;
}

}  // namespace rmx
