// quality.hpp -- the four quality figures of rmx_xcorr_batch_quality (include/rmx.h): coherence, peak-to-floor ratio, rms
// bandwidth and participation count of each output slot, from the two stored spectra of its pair alone (Parseval: the
// correlation vector is never stored and is not needed).
//
// A quality call runs the per-transform kernels, like a refined call (its spectra are in HBM when the pair kernels have
// finished).  Per chunk one k_quality launch follows the pair / final kernels on the same stream, IN FRONT OF k_refine
// (which overwrites peak) and before the next chunk's forward kernels overwrite the spectra.  Its work item is one output
// slot -- (window, pair), or (group, pair) of an integrated call, walking the group's K windows in order -- on one
// workgroup of kRefThreads threads:
//   - the two stored spectra are walked in STORAGE order with 16-byte loads at the same positions; every thread keeps five
//     float32 partial sums per window, in stored units (u = the forward kernels' power-of-two scale):
//         A = sum |X_i|^2    B = sum |X_j|^2    C = sum |X_i|^2 |X_j|^2    D = sum |X_i| |X_j|    F = sum (s / L)^2 |X_i| |X_j|
//     with s the signed index of the natural bin the stored position holds (ref_bin, refine.hpp); (s / L)^2 <= 1 / 4
//     whatever the length;
//   - the partial sums are reduced in the fixed tree of k_refine (xor shuffles within a wave, the waves in order through
//     LDS, no atomics): two identical calls give bit-identical outputs;
//   - thread 0 adds the per-window terms in window order -- EE += (A / (u^2 L)) (B / (u^2 L)), and C, D, F as they are --,
//     reads the coarse peak p0 from peak[slot], which the pair kernels just wrote, and writes the four values.  The
//     scales are exact powers of two, one factor per quantity: `sa` = 1 / (u^2 L) and `sc` = 1 / (u^4 L); rms_bw and
//     n_eff are ratios in which u cancels.
#pragma once

#include <hip/hip_runtime.h>

#include "refine.hpp"

namespace rmx {

struct QualityArgs {
    const float2* spec;     // the chunk's spectra, [item = window-in-chunk * n_buoys + buoy][L] in the layout's order
    const RefPair* pairs;   // [n_pairs] in output order
    long first_out;         // global index of the chunk's first output row (window, or group of an integrated call)
    int n_buoys, n_pairs;
    int logL;               // L = 2 N
    int row_bits;           // kRefRows: log2 of the rows per spectrum (L1); the row length is L >> row_bits
    int k;                  // windows per output row (1, or K of an integrated call)
    float sa;               // A, B in stored units -> energy of the window: 1 / (u^2 L)
    float sc;               // C in stored units -> sum over all L circular lags of |r|^2: 1 / (u^4 L)
};

constexpr int kQualSums = 5;   // A, B, C, D, F

// The trailing pack is empty for the plain kernel and <BandSet> for the banded one, as k_refine's (refine.hpp): output row
// gl is a virtual window, the spectra are real window gl / n_bands', and a position whose bin the band drops adds nothing
// -- in the weighted call it is a stored zero, which adds +0 to each of the five sums.  <LagBounds, Integrate, BandSet>:
// the banded pack of an integrated call, as k_refine's: row gl = group * n_bands + m walks its group's a.k windows, each
// under band (window, m), and thread 0 adds the per-window terms in window order as the plain kernel does.
// <CafWinner> (rmx_caf_batch_quality, caf_select.hpp): the plain body with operand j read from the de-rotated set of the
// slot's winning hypothesis; p0 is the winner's coarse peak, which the selection wrote.
template <int LAYOUT, class... P>
__global__ __launch_bounds__(kRefThreads) void k_quality(QualityArgs a, const float* __restrict__ peak, float* __restrict__ quality,
                                                         P... tail) {
    __shared__ float red[kRefWaves][kQualSums];
    const int tid = threadIdx.x;
    const int gl = blockIdx.x / a.n_pairs, q = blockIdx.x % a.n_pairs;   // output row inside the chunk, pair
    const long o = (a.first_out + gl) * (long)a.n_pairs + q;
    const int L = 1 << a.logL, N = L >> 1;
    [[maybe_unused]] const float2* spec_j = a.spec;
    if constexpr (kCafWinner<P...>) {
        const CafWinner cw = caf_winner_of(tail...);
        const int dw = cw.dop[o];
        if (cw.d >= 0 && dw != cw.d) return;   // (the whole workgroup: o is its slot)
        spec_j = cw.spec_j + (cw.d >= 0 ? 0L : dw * cw.hyp_items) * L;
    }
    const RefPair pr = a.pairs[q];
    const float inv_l = 1.0f / (float)L;   // a power of two
    float ee = 0.0f, sum_c = 0.0f, sum_d = 0.0f, sum_f = 0.0f;   // thread 0: over the windows, in window order
    [[maybe_unused]] XBand bd{0, 0u};
    [[maybe_unused]] long w_real = 0;
    if constexpr (kBanded<P...> && !kIntegrating<P...>) {
        const BandSet bs = band_set_of(tail...);
        bd = band_of_virtual(bs, gl);
        w_real = band_real_window(bs, gl);
    }
    for (int w = 0; w < a.k; ++w) {
        long wl = (long)gl * a.k + w;
        if constexpr (kBanded<P...> && kIntegrating<P...>) {   // row gl = group * n_bands + m: the group's window w under ITS band m
            const BandSet bs = band_set_of(tail...);
            const int g = gl / bs.n_bands;
            wl = (long)g * a.k + w;
            bd = band_of_window(bs, wl, gl - g * bs.n_bands);
        } else if constexpr (kBanded<P...>) {
            wl = w_real;   // (the banded pack of a call that is not integrated: a.k == 1)
        }
        const float4* xi = reinterpret_cast<const float4*>(a.spec + (wl * a.n_buoys + pr.i) * L);
        const float4* xj = reinterpret_cast<const float4*>(a.spec + (wl * a.n_buoys + pr.j) * L);
        if constexpr (kCafWinner<P...>) xj = reinterpret_cast<const float4*>(spec_j + (wl * a.n_buoys + pr.j) * L);
        float acc[kQualSums];
#pragma unroll
        for (int u = 0; u < kQualSums; ++u) acc[u] = 0.0f;
        for (int f = tid; f < (L >> 1); f += kRefThreads) {
            [[maybe_unused]] bool keep[2] = {true, true};
            if constexpr (kBanded<P...>) {
                keep[0] = xband_keeps(bd, ref_bin<LAYOUT>(2 * f, a.logL, a.row_bits), L - 1);
                keep[1] = xband_keeps(bd, ref_bin<LAYOUT>(2 * f + 1, a.logL, a.row_bits), L - 1);
                if (!(keep[0] || keep[1])) continue;
            }
            const float4 vi = xi[f], vj = xj[f];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                if constexpr (kBanded<P...>)
                    if (!keep[e]) continue;
                const float2 bi = e ? make_float2(vi.z, vi.w) : make_float2(vi.x, vi.y);
                const float2 bj = e ? make_float2(vj.z, vj.w) : make_float2(vj.x, vj.y);
                const int k = ref_bin<LAYOUT>(2 * f + e, a.logL, a.row_bits);
                const float t = (float)(k < N ? k : k - L) * inv_l;   // s / L, exact
                const float mi = bi.x * bi.x + bi.y * bi.y, mj = bj.x * bj.x + bj.y * bj.y;
                const float c2 = mi * mj;
                const float d = sqrtf(c2);   // |X_i| |X_j| = |P|
                acc[0] += mi;
                acc[1] += mj;
                acc[2] += c2;
                acc[3] += d;
                acc[4] += t * t * d;
            }
        }
        // fixed tree: xor butterflies inside each wave, then the waves in order
#pragma unroll
        for (int u = 0; u < kQualSums; ++u) {
            float v = acc[u];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
            if ((tid & 63) == 0) red[tid >> 6][u] = v;
        }
        __syncthreads();
        if (tid == 0) {
            float s[kQualSums];
#pragma unroll
            for (int u = 0; u < kQualSums; ++u) {
                s[u] = red[0][u];
#pragma unroll
                for (int v = 1; v < kRefWaves; ++v) s[u] += red[v][u];
            }
            ee += (s[0] * a.sa) * (s[1] * a.sa);
            sum_c += s[2];
            sum_d += s[3];
            sum_f += s[4];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const double p0 = (double)peak[o], p2 = p0 * p0;
    const double et = (double)sum_c * (double)a.sc, den = et - p2;
    double coh = 0.0, psr = 0.0;
    if (ee > 0.0f) {
        coh = p0 / sqrt((double)ee);
        coh = coh < 1.0 ? coh : 1.0;
    }
    if (p0 > 0.0) psr = den > 0.0 ? p2 * (double)(L - 1) / den : (double)INFINITY;
    float* out = quality + 4 * o;
    out[0] = (float)coh;
    out[1] = (float)psr;
    out[2] = sum_d > 0.0f ? (float)sqrt((double)sum_f / (double)sum_d) : 0.0f;
    out[3] = sum_c > 0.0f ? (float)((double)sum_d * (double)sum_d / (double)sum_c) : 0.0f;
}

}  // namespace rmx
