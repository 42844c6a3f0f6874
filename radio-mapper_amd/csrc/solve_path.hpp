// solve_path.hpp -- k_solve, the batched hyperbolic position solve of rmx_solve_batch; k_solve_plane and k_solve_fix, the
// surface-constrained walk and the information matrix at the fix of rmx_solve_batch_fix.
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

// ---- the fix with its information matrix (rmx_solve_batch_fix) -----------------------------------------
// A plane in ECEF: an origin o and two orthonormal directions e1, e2 (checked on the host); p(u) = o + u1 e1 + u2 e2.
// Passed to the kernels by value.
struct SolvePlane {
    double o[3], e1[3], e2[3];
};

// k_solve's walk with two unknowns: the position is held to the plane, the Jacobian row of a pair is (j . e1, j . e2)
// with k_solve's j, and the Levenberg-Marquardt rule is k_solve's written out for 2 x 2.  One thread per window, as there.
// The start is the centroid (summed as k_solve sums it) projected onto the plane; the step length is |du|, which is the
// step in metres because e1 and e2 are orthonormal.  pos is p(u) where cost was evaluated.
__global__ __launch_bounds__(64) void k_solve_plane(const double* __restrict__ buoy_xyz, int n_buoys,
                                                    const int* __restrict__ pairs, int n_pairs,
                                                    const int* __restrict__ lag_int, const float* __restrict__ lag_frac,
                                                    const float* __restrict__ weight, double metres_per_sample,
                                                    SolvePlane pl, int n_windows, int max_iter,
                                                    double* __restrict__ pos, double* __restrict__ cost,
                                                    int* __restrict__ iters) {
#pragma clang fp contract(off)   // same roundings as the numpy restatement (tests/solve_fix_ref.py)
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
    double cx = 0, cy = 0, cz = 0;
    for (int b = 0; b < n_buoys; ++b) { cx += sb[3 * b]; cy += sb[3 * b + 1]; cz += sb[3 * b + 2]; }
    cx /= n_buoys; cy /= n_buoys; cz /= n_buoys;
    double u1 = (cx - pl.o[0]) * pl.e1[0] + (cy - pl.o[1]) * pl.e1[1] + (cz - pl.o[2]) * pl.e1[2];
    double u2 = (cx - pl.o[0]) * pl.e2[0] + (cy - pl.o[1]) * pl.e2[1] + (cz - pl.o[2]) * pl.e2[2];
    double px = pl.o[0] + u1 * pl.e1[0] + u2 * pl.e2[0];
    double py = pl.o[1] + u1 * pl.e1[1] + u2 * pl.e2[1];
    double pz = pl.o[2] + u1 * pl.e1[2] + u2 * pl.e2[2];
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
        double a00 = 0, a01 = 0, a11 = 0, g0 = 0, g1 = 0;
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
            const double j1 = jx * pl.e1[0] + jy * pl.e1[1] + jz * pl.e1[2];
            const double j2 = jx * pl.e2[0] + jy * pl.e2[1] + jz * pl.e2[2];
            const double ww = wg ? (double)wg[q] : 1.0;
            a00 += ww * j1 * j1; a01 += ww * j1 * j2; a11 += ww * j2 * j2;
            g0 += ww * j1 * r; g1 += ww * j2 * r;
        }
        // (A + lam diag A) delta = -g by Cholesky; a failed factorisation counts as a rejected step
        const double d00 = a00 * (1.0 + lam), d11 = a11 * (1.0 + lam);
        bool ok = d00 > 0.0;
        const double l00 = sqrt(ok ? d00 : 1.0);
        const double l10 = a01 / l00;
        const double t11 = d11 - l10 * l10;
        ok = ok && t11 > 0.0;
        const double l11 = sqrt(ok ? t11 : 1.0);
        bool accepted = false;
        double dn = 0.0;
        if (ok) {
            const double y0 = -g0 / l00;
            const double y1 = (-g1 - l10 * y0) / l11;
            const double d2 = y1 / l11;
            const double d1 = (y0 - l10 * d2) / l00;
            const double t1 = u1 + d1, t2 = u2 + d2;
            const double tx = pl.o[0] + t1 * pl.e1[0] + t2 * pl.e2[0];
            const double ty = pl.o[1] + t1 * pl.e1[1] + t2 * pl.e2[1];
            const double tz = pl.o[2] + t1 * pl.e1[2] + t2 * pl.e2[2];
            const double fn = f_at(tx, ty, tz);
            if (fn < f) {
                u1 = t1; u2 = t2;
                px = tx; py = ty; pz = tz;
                f = fn;
                accepted = true;
                dn = sqrt(d1 * d1 + d2 * d2);
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

// At the fix: one more Jacobian pass at pos[w], without damping.  info = J^T W J (PLANE: 11 12 22 in plane coordinates;
// otherwise xx xy xz yy yz zz in ECEF), cov = its inverse through Cholesky in the same layout, resid[w][q] = the pair's
// residual in metres (resid == nullptr: not written).  A pivot <= kSolveSingular * its own diagonal entry, or one that is
// not finite, makes the information singular: cov = +inf on the diagonal, 0 off it.  An info entry that is not finite
// (pos exactly on a buoy of a pair: 0 / 0 in its Jacobian row) gives info = 0 and the singular cov: no output is NaN.
constexpr double kSolveSingular = 1e-12;
template <bool PLANE>
__global__ __launch_bounds__(64) void k_solve_fix(const double* __restrict__ buoy_xyz, int n_buoys,
                                                  const int* __restrict__ pairs, int n_pairs,
                                                  const int* __restrict__ lag_int, const float* __restrict__ lag_frac,
                                                  const float* __restrict__ weight, double metres_per_sample,
                                                  SolvePlane pl, int n_windows, const double* __restrict__ pos,
                                                  double* __restrict__ info, double* __restrict__ cov,
                                                  double* __restrict__ resid) {
#pragma clang fp contract(off)
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
    double* rs = resid ? resid + (long)w * n_pairs : nullptr;
    const double px = pos[3 * (long)w], py = pos[3 * (long)w + 1], pz = pos[3 * (long)w + 2];
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
    for (int q = 0; q < n_pairs; ++q) {
        const double* b1 = sb + 3 * spair[2 * q];
        const double* b2 = sb + 3 * spair[2 * q + 1];
        const double v1x = px - b1[0], v1y = py - b1[1], v1z = pz - b1[2];
        const double v2x = px - b2[0], v2y = py - b2[1], v2z = pz - b2[2];
        const double n1 = sqrt(v1x * v1x + v1y * v1y + v1z * v1z);
        const double n2 = sqrt(v2x * v2x + v2y * v2y + v2z * v2z);
        if (rs) rs[q] = n2 - n1 - ((double)li[q] + (double)lf[q]) * metres_per_sample;
        const double jx = v2x / n2 - v1x / n1, jy = v2y / n2 - v1y / n1, jz = v2z / n2 - v1z / n1;
        const double ww = wg ? (double)wg[q] : 1.0;
        if (PLANE) {
            const double j1 = jx * pl.e1[0] + jy * pl.e1[1] + jz * pl.e1[2];
            const double j2 = jx * pl.e2[0] + jy * pl.e2[1] + jz * pl.e2[2];
            a00 += ww * j1 * j1; a01 += ww * j1 * j2; a11 += ww * j2 * j2;
        } else {
            a00 += ww * jx * jx; a01 += ww * jx * jy; a02 += ww * jx * jz;
            a11 += ww * jy * jy; a12 += ww * jy * jz; a22 += ww * jz * jz;
        }
    }
    const double inf = __builtin_huge_val();
    if (PLANE) {
        double* io = info + 3 * (long)w;
        double* co = cov + 3 * (long)w;
        const bool fin = __builtin_isfinite(a00) && __builtin_isfinite(a01) && __builtin_isfinite(a11);
        bool ok = fin && a00 > kSolveSingular * a00;
        const double l00 = sqrt(ok ? a00 : 1.0);
        const double l10 = a01 / l00;
        const double t11 = a11 - l10 * l10;
        ok = ok && t11 > kSolveSingular * a11 && __builtin_isfinite(t11);
        const double l11 = sqrt(ok ? t11 : 1.0);
        const double m00 = 1.0 / l00, m11 = 1.0 / l11;
        const double m10 = -(l10 * m00) / l11;
        io[0] = fin ? a00 : 0.0; io[1] = fin ? a01 : 0.0; io[2] = fin ? a11 : 0.0;
        co[0] = ok ? m00 * m00 + m10 * m10 : inf;
        co[1] = ok ? m10 * m11 : 0.0;
        co[2] = ok ? m11 * m11 : inf;
    } else {
        double* io = info + 6 * (long)w;
        double* co = cov + 6 * (long)w;
        const bool fin = __builtin_isfinite(a00) && __builtin_isfinite(a01) && __builtin_isfinite(a02) &&
                         __builtin_isfinite(a11) && __builtin_isfinite(a12) && __builtin_isfinite(a22);
        bool ok = fin && a00 > kSolveSingular * a00;
        const double l00 = sqrt(ok ? a00 : 1.0);
        const double l10 = a01 / l00, l20 = a02 / l00;
        const double t11 = a11 - l10 * l10;
        ok = ok && t11 > kSolveSingular * a11 && __builtin_isfinite(t11);
        const double l11 = sqrt(ok ? t11 : 1.0);
        const double l21 = (a12 - l20 * l10) / l11;
        const double t22 = a22 - l20 * l20 - l21 * l21;
        ok = ok && t22 > kSolveSingular * a22 && __builtin_isfinite(t22);
        const double l22 = sqrt(ok ? t22 : 1.0);
        // M = L^-1 (lower triangular), cov = M^T M
        const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
        const double m10 = -(l10 * m00) / l11;
        const double m21 = -(l21 * m11) / l22;
        const double m20 = -(l20 * m00 + l21 * m10) / l22;
        io[0] = fin ? a00 : 0.0; io[1] = fin ? a01 : 0.0; io[2] = fin ? a02 : 0.0;
        io[3] = fin ? a11 : 0.0; io[4] = fin ? a12 : 0.0; io[5] = fin ? a22 : 0.0;
        co[0] = ok ? m00 * m00 + m10 * m10 + m20 * m20 : inf;
        co[1] = ok ? m10 * m11 + m20 * m21 : 0.0;
        co[2] = ok ? m20 * m22 : 0.0;
        co[3] = ok ? m11 * m11 + m21 * m21 : inf;
        co[4] = ok ? m21 * m22 : 0.0;
        co[5] = ok ? m22 * m22 : inf;
    }
}

}  // namespace rmx
