// refine.hpp -- the fine lag search of rmx_xcorr_batch_refined (include/rmx.h): the band-limited interpolant of the
// correlation on a grid of 1 / U samples around the integer peak, evaluated straight from the cross-spectrum.
//
// A refined call runs the per-transform kernels (its spectra are in HBM when the pair kernels have finished).  Per chunk
// one k_refine launch follows the pair / final kernels, on the same stream, before the next chunk's forward kernels
// overwrite the spectra.  Its work item is one output slot -- (window, pair), or (group, pair) of an integrated call,
// walking the group's K windows in order -- on one workgroup of kRefThreads threads:
//   - lag0 is read from lag_int[slot], which the pair kernels just wrote; the coarse rule is not touched;
//   - the two stored spectra are walked in STORAGE order with 16-byte loads at the same positions; every stored
//     position is mapped to its natural bin k by the map of the forward kernel that wrote it (xspec_weight.hpp), and
//     P = X_j conj(X_i) is rotated to the 2 U + 1 lags lag0 + u / U: with s the signed index of k,
//         base = ((k lag0) mod L) / L turns     (k = s mod L and lag0 is an integer)
//         step = s / (U L) turns                (|s| <= N: exact in float32)
//     both exact rationals with power-of-two denominators, reduced in integers and handed to sincospif as multiples of
//     pi -- 2 pi s t / L is never formed in float.  P base is rotated outward from u = 0 by the step, U complex
//     multiplies each way, and added into 2 U + 1 complex partial sums in registers (U is a template argument);
//   - the partial sums are reduced in a fixed tree (xor shuffles within a wave, LDS across the waves, no atomics), so
//     two identical calls give bit-identical outputs; thread u then adds |r_w(lag0 + u / U)|^2 into its float32 sum,
//     window after window in window order;
//   - thread 0 resolves u*, the parabola and the carry into lag_int in double and overwrites the three outputs.
// The stored spectra carry the forward kernels' power-of-two scale; `scale` = (1 / L) / unit^2 is exact.
#pragma once

#include <hip/hip_runtime.h>

#include "caf_select.hpp"
#include "lag_bounds.hpp"
#include "xspec_bands.hpp"
#include "xspec_weight.hpp"

namespace rmx {

constexpr int kRefThreads = 256;
constexpr int kRefWaves = kRefThreads / 64;

// which forward kernel stored the spectra
enum RefLayout { kRefKfwd = 0, kRefSmall = 1, kRefRows = 2 };

struct RefPair {
    int i, j;
};

struct RefineArgs {
    const float2* spec;     // the chunk's spectra, [item = window-in-chunk * n_buoys + buoy][L] in the layout's order
    const RefPair* pairs;   // [n_pairs] in output order
    LagBounds lb;           // b == nullptr: the full interval; else the call's intervals (w is the global window / group)
    long first_out;         // global index of the chunk's first output row (window, or group of an integrated call)
    int n_buoys, n_pairs;
    int logL;               // L = 2 N
    int row_bits;           // kRefRows: log2 of the rows per spectrum (L1); the row length is L >> row_bits
    int k;                  // windows per output row (1, or K of an integrated call)
    float scale;            // |sum| -> |r|: (1 / L) / (forward scale)^2, a power of two
};

// natural bin of stored complex position pos (0 .. L-1) of one spectrum
template <int LAYOUT>
__device__ __forceinline__ int ref_bin(int pos, int logL, int row_bits) {
    if constexpr (LAYOUT == kRefKfwd) {
        const int f = pos >> 1;   // float4 index j * kThreads + t: slots 2 j, 2 j + 1 of thread t
        return xbin_kfwd(f & 1, (f & 511) >> 1) + kXbinKfwdSlot * (2 * (f >> 9) + (pos & 1));
    } else if constexpr (LAYOUT == kRefSmall) {
        return xbin_small(pos, logL);
    } else {
        const int logR = logL - row_bits;
        return xbin_rows(xbin_rows_k1(pos >> logR, row_bits), pos & ((1 << logR) - 1), row_bits, logR);
    }
}

// The rotation steps of the banded k_refine in the form hipcc compiles the plain kernel's to.  Each component of a step
// is a sum of two products, one of which is rounded and one fused into the multiply-add; which one is the compiler's
// choice (-ffp-contract), it depends on the order in which the backend meets the nodes, and it fell differently in the
// banded instantiation: last-bit differences from the single-band call.  The plain kernel's forms are stated here with the
// contraction off (tests/test_gpu_bands_quality.py holds the two kernels together, every U on every layout).  The
// <CafWinner> instantiation takes them too: left to the backend, its first step rounded sc * c0.x and fused ss * c0.y
// (tests/test_gpu_caf_quality.py holds it to the plain kernel bit for bit):
//   u = 1, up and dn both from c0, sharing their products:   ss * c0 rounded, sc * c0 fused
//   u > 1:   up.x, dn.x, dn.y: the ss product rounded, the sc product fused;   up.y: sc * up.y rounded, ss * up.x fused
__device__ __forceinline__ void ref_first_step(const float2 c0, float ss, float sc, float2& up, float2& dn) {
#pragma clang fp contract(off)
    const float sx = ss * c0.x, sy = ss * c0.y;
    up = make_float2(__builtin_fmaf(sc, c0.x, -sy), __builtin_fmaf(sc, c0.y, sx));
    dn = make_float2(__builtin_fmaf(sc, c0.x, sy), __builtin_fmaf(sc, c0.y, -sx));
}
__device__ __forceinline__ void ref_next_step(float ss, float sc, float2& up, float2& dn) {
#pragma clang fp contract(off)
    const float uy = ss * up.y, ux = sc * up.y, dy = ss * dn.y, dx = ss * dn.x;
    up = make_float2(__builtin_fmaf(sc, up.x, -uy), __builtin_fmaf(ss, up.x, ux));
    dn = make_float2(__builtin_fmaf(sc, dn.x, dy), __builtin_fmaf(sc, dn.y, -dx));
}

// The trailing pack is empty for the plain kernel and <BandSet> for the banded one (rmx_xcorr_batch_bands_quality,
// xspec_bands.hpp): the output row gl is then a VIRTUAL window -- the spectra are those of real window gl / n_bands, the
// band is band_of_virtual(gl), the outputs and the lag interval are row gl's --, a.k is 1, and a stored position whose
// natural bin the band drops contributes nothing: a 16-byte load both of whose bins are dropped is not issued and its
// sincospif pairs are not evaluated.  The thread-to-position map, the order of a thread's additions and the reduction
// tree are the plain kernel's, and what is skipped is what the weighted call adds as +-0 to sums that start at +0:
// slot (w, m, q) carries the bits of the refined call with band[w][m].
// <LagBounds, Integrate, BandSet> is the banded pack of an integrated call (rmx_xcorr_batch_bands_integrated): output row
// gl = group * n_bands + m walks the a.k real windows of its group in window order, each under band (window, m); the sums,
// the fixed tree and the tap rule are those of the plain kernel with a.k > 1.  Of that pack only
// the band set is read: the lag intervals and K are a.lb and a.k.
// <CafWinner> (rmx_caf_batch_quality, caf_select.hpp): the plain body -- a band is stored masked --, with operand j read
// from the de-rotated set of the slot's winning hypothesis; lag0 is the winner's coarse lag, which the selection wrote.
template <int U, int LAYOUT, class... P>
__global__ __launch_bounds__(kRefThreads) void k_refine(RefineArgs a, int* __restrict__ lag_int, float* __restrict__ lag_frac,
                                                        float* __restrict__ peak, P... tail) {
    constexpr int T = 2 * U + 1;
    __shared__ float red[kRefWaves][2 * T];
    __shared__ float taps[T];
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
    const int lag0 = lag_int[o];
    const RefPair pr = a.pairs[q];
    const float inv_n = 1.0f / (float)N, inv_un = 1.0f / ((float)N * (float)U);   // powers of two
    float fsum = 0.0f;   // thread u < T: sum over the windows of |r_w(lag0 + (u - U) / U)|^2, unscaled
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
        float2 acc[T];
#pragma unroll
        for (int u = 0; u < T; ++u) acc[u] = make_float2(0.0f, 0.0f);
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
                const int s = k < N ? k : k - L;
                const unsigned m = ((unsigned)k * (unsigned)lag0) & (unsigned)(L - 1);   // (k lag0) mod L: L divides 2^32
                float bs, bc, ss, sc;
                sincospif((float)m * inv_n, &bs, &bc);      // base: 2 m / L half turns
                sincospif((float)s * inv_un, &ss, &sc);     // step: 2 s / (U L) half turns
                const float2 p = make_float2(bj.x * bi.x + bj.y * bi.y, bj.y * bi.x - bj.x * bi.y);   // X_j conj(X_i)
                const float2 c0 = make_float2(p.x * bc - p.y * bs, p.x * bs + p.y * bc);
                acc[U].x += c0.x;
                acc[U].y += c0.y;
                float2 up = c0, dn = c0;
#pragma unroll
                for (int u = 1; u <= U; ++u) {
                    if constexpr (kBanded<P...> || kCafWinner<P...>) {
                        if (u == 1) ref_first_step(c0, ss, sc, up, dn);
                        else ref_next_step(ss, sc, up, dn);
                    } else {
                        up = make_float2(up.x * sc - up.y * ss, up.x * ss + up.y * sc);
                        dn = make_float2(dn.x * sc + dn.y * ss, dn.y * sc - dn.x * ss);
                    }
                    acc[U + u].x += up.x;
                    acc[U + u].y += up.y;
                    acc[U - u].x += dn.x;
                    acc[U - u].y += dn.y;
                }
            }
        }
        // fixed tree: xor butterflies inside each wave, then the waves in order
#pragma unroll
        for (int u = 0; u < T; ++u) {
            float re = acc[u].x, im = acc[u].y;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                re += __shfl_xor(re, d, 64);
                im += __shfl_xor(im, d, 64);
            }
            if ((tid & 63) == 0) {
                red[tid >> 6][2 * u] = re;
                red[tid >> 6][2 * u + 1] = im;
            }
        }
        __syncthreads();
        if (tid < T) {
            float re = red[0][2 * tid], im = red[0][2 * tid + 1];
#pragma unroll
            for (int v = 1; v < kRefWaves; ++v) {
                re += red[v][2 * tid];
                im += red[v][2 * tid + 1];
            }
            fsum += re * re + im * im;   // in window order
        }
        __syncthreads();
    }
    if (tid < T) taps[tid] = sqrtf(fsum) * a.scale;
    __syncthreads();
    if (tid != 0) return;
    int lo = -(N - 1), hi = N - 1;
    if (a.lb.b) {
        const int* p = a.lb.b + (a.first_out + gl) * a.lb.wstride + 2 * q;
        lo = p[0];
        hi = p[1];
    }
    // admitted: lo <= lag0 + u / U <= hi, i.e. every u >= 0 (<= 0) unless lag0 sits on hi (lo)
    const int umin = lag0 > lo ? -U : 0, umax = lag0 < hi ? U : 0;
    int best = 0;
    float fb = taps[U];
    for (int d = 1; d <= U; ++d) {   // equal values: the smallest |u|, then the negative one
        if (-d >= umin && taps[U - d] > fb) { fb = taps[U - d]; best = -d; }
        if (d <= umax && taps[U + d] > fb) { fb = taps[U + d]; best = d; }
    }
    double dd = 0.0;
    if (best - 1 >= umin && best + 1 <= umax) {
        const double ta = (double)taps[U + best - 1], tb = (double)fb, tc = (double)taps[U + best + 1];
        const double den = ta - 2.0 * tb + tc;
        dd = den == 0.0 ? 0.0 : 0.5 * (ta - tc) / den;
    }
    const double delta = ((double)best + dd) / (double)U;
    const int n = delta > 0.5 ? 1 : (delta < -0.5 ? -1 : 0);
    lag_int[o] = lag0 + n;
    lag_frac[o] = (float)(delta - (double)n);
    peak[o] = fb;
}

}  // namespace rmx
