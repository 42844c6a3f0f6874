// pair4096.hpp -- the per-transform kernels of N = 4096 (L = 8192): k_fwd, one workgroup per (window, buoy), stores the
// forward spectrum in the register layout of the pair kernels; k_pair_str / k_pair_res, one workgroup per (window, group
// of pairs), load two spectra, multiply in registers, inverse transform, |.|^2, workgroup argmax with numpy
// tie-breaking, 3-tap parabola, 12 bytes out per pair-window.  Launched by fwd4096 / pairs4096 (rmx_hip.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "fft_r16.hpp"
#include "generic_path.hpp"   // gen::rot_mul
#include "host_plan.hpp"      // PairItem
#include "integrate.hpp"
#include "kwin.hpp"           // the LDS carve (kLdsXchg, kLdsTw2, kLdsBytes) and the table loaders
#include "lag_bounds.hpp"
#include "xspec_bands.hpp"
#include "xspec_weight.hpp"

namespace rmx {

// ------------------------------------------------------------------------------------------------
// Forward spectra.  grid = n_items workgroups of 512; item = wl * B + b inside the chunk.
//   spec layout: [item][j = 0..7][t = 0..511] float4 = bins of slots (2j, 2j+1) of thread t,
//   scaled by `scale` (a power of two; the pair kernel's product then carries 1/L exactly).
template <bool U8, class... WT>   // WT: empty, or one XWeight (the weighted instantiation, xspec_weight.hpp)
__global__ __launch_bounds__(kThreads, 4) void k_fwd(const void* __restrict__ iq_v, float4* __restrict__ spec,
                                                     const float4* __restrict__ tw1_g,
                                                     const float2* __restrict__ tw2_g, long first_item,
                                                     float scale, const float2* __restrict__ rot, int wrap_items,
                                                     WT... wt_pack) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* xl = reinterpret_cast<float2*>(smem);
    float2* tw2_lds = reinterpret_cast<float2*>(smem + kLdsXchg);
    const int t = threadIdx.x;
    const int p = t & 1, u = t >> 1;
    // wrap_items > 0 (rmx_caf_batch, all hypotheses in one launch): workgroup b transforms real item b % wrap_items
    // de-rotated by hypothesis b / wrap_items; its spectrum still goes to slot b
    const long item = first_item + (wrap_items > 0 ? (long)(blockIdx.x % (unsigned)wrap_items) : (long)blockIdx.x);
    if (wrap_items > 0 && rot) rot += (size_t)(blockIdx.x / (unsigned)wrap_items) * kM;

    load_tw2_to_lds(tw2_lds, tw2_g, t);
    float2 tw1[16];
    load_tw1(tw1, tw1_g, t);

    float2 v[16];
    if constexpr (U8) {
        const uchar2* x = reinterpret_cast<const uchar2*>(iq_v) + item * kM;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const uchar2 b = x[q * 256 + u];
            v[q] = make_float2((float)b.x - 127.5f, (float)b.y - 127.5f);
        }
    } else {
        const float2* x = reinterpret_cast<const float2*>(iq_v) + item * kM;
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = x[q * 256 + u];
    }
    if (rot) {   // rmx_caf_batch: the window de-rotated by this Doppler hypothesis (gen::rot_mul: nothing fused)
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = gen::rot_mul(v[q], rot[q * 256 + u]);
    }
    // odd sub-transform: x[n] * W_L^n = x * W32^q * W_L^u ; W_L^u is folded into tw1 (odd lanes)
    if (p) {
#pragma unroll
        for (int q = 1; q < 16; ++q) v[q] = cmul(v[q], w32(q));
    }
    dft16(v);        // n2 -> k0
    mul_tw1(v, tw1); // W_M^(u*k0) [* W_L^u on odd lanes]
    xchg_a_write(xl, v, t);
    __syncthreads();
    xchg_b_read(xl, v, t);
    dft16(v);                         // n1 -> k1
    mul_tw2(v, tw2_lds, u & 15);      // W_256^(n0*k1)
    xchg_bc_write_b(xl, v, t);        // own half-wave region: no barrier
    wave_lds_fence();
    xchg_bc_read_c(xl, v, t);
    dft16(v);                         // n0 -> k2
    if constexpr (sizeof...(WT) > 0) {   // weighted call; item is the REAL global item under wrap_items too: its window's band
        const XWeight wt = xweight_of(wt_pack...);
        const XBand bd = xband_of(wt, item / wt.n_buoys);
        // role C (fft_r16.hpp): u = 16 k0 + k1, slot s = k2 -> natural bin 2 (k0 + 16 k1 + 256 s) + p
        const int kb = RMX_XBIN_KFWD(p, u);   // (xspec_weight.hpp: the map k_refine reads the spectra back with)
#pragma unroll
        for (int s = 0; s < 16; ++s) v[s] = xweight_apply(wt, bd, kb + kXbinKfwdSlot * s, kL - 1, v[s]);
    }
    float4* out = spec + (long)blockIdx.x * (8 * kThreads);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        out[j * kThreads + t] = make_float4(v[2 * j].x * scale, v[2 * j].y * scale,
                                            v[2 * j + 1].x * scale, v[2 * j + 1].y * scale);
}

// ------------------------------------------------------------------------------------------------
// Pair kernel.  grid = n_windows_in_chunk * n_parts; each workgroup walks items[part_begin..end).
//   out arrays are indexed [(first_window + wl) * n_pairs + item.out].
// Streaming variant (k_pair_str, option "resident" = 0): two workgroups per CU (<= 128 VGPRs); TW1,
// X_i and X_j are re-read every pair.  The resident variant is k_pair_res below.
template <bool BOUNDED, class... BS>   // BS: empty, or one BandSet (the banded instantiations, xspec_bands.hpp)
__device__ __forceinline__ void pair_body(const float4* __restrict__ spec, const float4* __restrict__ spec_j,
                                          const float4* __restrict__ tw1_g,
                                          const float2* __restrict__ tw2_g, const PairItem* __restrict__ items,
                                          const int* __restrict__ part_begin, int n_parts, int n_buoys,
                                          int n_pairs, int xcd_map, long first_window, float out_scale,
                                          int* __restrict__ lag_int, float* __restrict__ lag_frac,
                                          float* __restrict__ peak, int i_wrap, LagBounds lb, BS... bs_pack) {
    constexpr bool BANDED = sizeof...(BS) > 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* xl = reinterpret_cast<float2*>(smem);
    float2* tw2_lds = reinterpret_cast<float2*>(smem + kLdsXchg);
    float* red_max = reinterpret_cast<float*>(smem + kLdsXchg + kLdsTw2);      // [8]
    int* red_k = reinterpret_cast<int*>(smem + kLdsXchg + kLdsTw2 + 32);       // [1]
    float* red_tap = reinterpret_cast<float*>(smem + kLdsXchg + kLdsTw2 + 48); // [3]

    const int t = threadIdx.x;
    const int p = t & 1, u = t >> 1;
    const int lane = t & 63, wave = t >> 6;

    // blockIdx -> (window, part).  Workgroups of one window share its spectra through the XCD's
    // L2, so keep them on one XCD (blocks b and b+8 share an XCD) and adjacent in dispatch order.
    // Placement only changes speed, never results.
    int wl, part;
    {
        const int b = blockIdx.x;
        if (xcd_map) {
            const int xcd = b & 7, s = b >> 3;
            wl = (s / n_parts) * 8 + xcd;
            part = s % n_parts;
        } else {
            wl = b / n_parts;
            part = b % n_parts;
        }
    }

    load_tw2_to_lds(tw2_lds, tw2_g, t);
    __syncthreads();

    const float sgn = p ? -1.0f : 1.0f;
    const int it_begin = part_begin[part];
    const int it_end = part_begin[part + 1];
    // banded: wl is a VIRTUAL window (real window wl / n_bands, band wl % n_bands); both spectra are the real window's,
    // and bit s of `keep` says whether this thread's slot s lies in the band (role C: xspec_weight.hpp's k_fwd map)
    // rmx_caf_batch_bands, all hypotheses in one launch (i_wrap > 0, in virtual windows): wl = (hypothesis * windows +
    // window) * n_bands + band; operand j is at wl / n_bands in the de-rotated set, operand i and the band are those of
    // virtual window wl % i_wrap = window * n_bands + band.  All of it scalar, once per workgroup.
    int wr = wl;
    [[maybe_unused]] int wr_i = wl;
    [[maybe_unused]] unsigned keep = 0xffffu;
    if constexpr (BANDED) {
        const BandSet bs = band_set_of(bs_pack...);
        const int vi = i_wrap > 0 ? wl % i_wrap : wl;
        wr = band_real_window(bs, wl);
        wr_i = band_real_window(bs, vi);
        const XBand bd = band_of_virtual(bs, vi);
        const int kb = RMX_XBIN_KFWD(p, u);
        keep = 0u;
#pragma unroll
        for (int s = 0; s < 16; ++s) keep |= (xband_keeps(bd, kb + kXbinKfwdSlot * s, kL - 1) ? 1u : 0u) << s;
    }
    const long wbase = (long)wr * n_buoys;
    long wbase_i;
    if constexpr (BANDED) wbase_i = (long)wr_i * n_buoys;
    else wbase_i = (long)(i_wrap > 0 ? wl % i_wrap : wr) * n_buoys;   // (rmx_caf_batch: wl = hypothesis * windows + window)
    float4 sa[8], sb[8];   // X_i (anchor) and X_j of the pair about to be processed
    PairItem pi = items[it_begin < it_end ? it_begin : 0];
    if (it_begin < it_end) {
        const float4* xi = spec + (wbase_i + pi.i) * (8 * kThreads);
        const float4* xj = spec_j + (wbase + pi.j) * (8 * kThreads);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sa[j] = xi[j * kThreads + t];
            sb[j] = xj[j * kThreads + t];
        }
    }
    for (int it = it_begin; it < it_end; ++it) {
        const int out_idx = pi.out;
        float2 v[16];
        // R = X_j * conj(X_i), written (im, re)-swapped: the forward blocks below then compute the
        // inverse transform (swap o F o swap = conj F).
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 a = sa[j];
            const float4 b = sb[j];
            v[2 * j] = make_float2(b.y * a.x - b.x * a.y, b.x * a.x + b.y * a.y);
            v[2 * j + 1] = make_float2(b.w * a.z - b.z * a.w, b.z * a.z + b.w * a.w);
        }
        if constexpr (BANDED) {       // the band: a dropped bin's product is +0
#pragma unroll
            for (int s = 0; s < 16; ++s)
                if (!((keep >> s) & 1u)) v[s] = make_float2(0.0f, 0.0f);
        }
        dft16(v);                     // k2 -> n0   (role C)
        mul_tw2(v, tw2_lds, u & 15);  // W_256^(k1*n0)
        xchg_bc_write_c(xl, v, t);
        wave_lds_fence();
        xchg_bc_read_b(xl, v, t);
        dft16(v);                     // k1 -> n1   (role B)
        float2 tw1s[16];
        {
            // TW1 re-read every pair (64 KiB per workgroup from L2); the pointer is laundered so
            // that the loads stay here, in flight across the exchange.
            const float4* twp = tw1_g;
            asm volatile("" : "+s"(twp));
            load_tw1(tw1s, twp, t);
        }
        xchg_b_write(xl, v, t);       // into this half wave's own region: no barrier needed before
        __syncthreads();
        xchg_a_read(xl, v, t);
        mul_tw1(v, tw1s);             // W_M^(u*k0) [* W_L^u odd]
        dft16(v);                     // k0 -> n2   (role A): lane holds e[n] (p=0) or o[n]*W_L^u (p=1)
        if (p) {
#pragma unroll
            for (int q = 1; q < 16; ++q) v[q] = cmul(v[q], w32(q));
        }
        // last radix-2 stage across the lane pair: even lane r[n] = e + o', odd lane r[n+M] = e - o'
        float mag[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float rx = sgn * v[q].x + dpp_xor1(v[q].x);
            const float ry = sgn * v[q].y + dpp_xor1(v[q].y);
            mag[q] = rx * rx + ry * ry;
        }
        {
            if (it + 1 < it_end) {
                pi = items[it + 1];
                const float4* xi = spec + (wbase_i + pi.i) * (8 * kThreads);
                const float4* xj = spec_j + (wbase + pi.j) * (8 * kThreads);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    sa[j] = xi[j * kThreads + t];
                    sb[j] = xj[j * kThreads + t];
                }
            }
        }
        // 'full' order index of slot q: even lanes lag tau = n >= 0 -> k = n + M - 1;
        // odd lanes tau = n - M -> k = n - 1 (n = 0, i.e. tau = -M, is not part of 'full').
        if (p && u == 0) mag[0] = -1.0f;
        int klo = 0, khi = 2 * kM - 2;
        if constexpr (BOUNDED) {   // lag window: |r|^2 outside it -> the same sentinel (lag_bounds.hpp)
            // (one launch for all hypotheses: the bounds are the REAL window's, wl % i_wrap; the output slot stays virtual)
            lag_window(lb, first_window + (i_wrap > 0 ? wl % i_wrap : wl), out_idx, kM - 1, klo, khi);
            const int kb = p ? (u - 1) : (u + kM - 1);
#pragma unroll
            for (int q = 0; q < 16; ++q) mag[q] = lag_mask(mag[q], kb + q * 256, klo, khi);
        }
        float tmax = mag[0];
#pragma unroll
        for (int q = 1; q < 16; ++q) tmax = fmaxf(tmax, mag[q]);
        float wmax = tmax;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, off, 64));
        if (lane == 0) red_max[wave] = wmax;
        if (t == 0) *red_k = 0x7fffffff;
        __syncthreads();
        float gmax = red_max[0];
#pragma unroll
        for (int w = 1; w < 8; ++w) gmax = fmaxf(gmax, red_max[w]);
        const int kbase = p ? (u - 1) : (u + kM - 1);
        if (tmax == gmax) {
            int kmin = 0x7fffffff;
#pragma unroll
            for (int q = 15; q >= 0; --q)
                if (mag[q] == gmax) kmin = kbase + q * 256;
            atomicMin(red_k, kmin);
        }
        __syncthreads();
        const int kstar = *red_k;
        // owners of taps k*-1, k*, k*+1 publish |r| (scipy scaling)
#pragma unroll
        for (int d = -1; d <= 1; ++d) {
            const int kk = kstar + d;
            if (kk >= 0 && kk <= 2 * kM - 2) {
                const int par = (kk >= kM - 1) ? 0 : 1;
                const int n = par ? (kk + 1) : (kk - (kM - 1));
                if (p == par && u == (n & 255)) {
                    const int qo = n >> 8;
                    float val = 0.0f;
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (q == qo) val = mag[q];
                    red_tap[d + 1] = sqrtf(val) * out_scale;
                }
            }
        }
        __syncthreads();
        if (t == 0) {
            const double b = (double)red_tap[1];
            double frac = 0.0;
            if (kstar > klo && kstar < khi) {   // (klo = 0, khi = 2M - 2 unbounded)
                const double a = (double)red_tap[0], c = (double)red_tap[2];
                const double den = a - 2.0 * b + c;
                if (den != 0.0) frac = 0.5 * (a - c) / den;
            }
            const long o = (first_window + wl) * (long)n_pairs + out_idx;
            lag_int[o] = kstar - (kM - 1);
            lag_frac[o] = (float)frac;
            peak[o] = (float)b;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The integrating instantiation of k_pair_str (integrate.hpp).  grid = groups_in_chunk * n_parts; a work item is
// (group, pair): the workgroup walks the group's K windows -- product, the three radix-16 passes, |.|^2 as in pair_body --
// and adds each window's mag[16] into acc[16], in window order; masking, argmax, tap publication and parabola then run
// once, on acc.  The next window's spectra (or the next pair's first window's) are requested where pair_body requests
// the next pair's.  With the 16 sums on top of pair_body's registers the kernel does not fit 128 VGPRs (pair_body itself
// spills there), so this instantiation is built for two waves per SIMD, one workgroup per CU, like k_pair_res, and keeps
// TW1 in registers as that kernel does.  One more barrier per window than pair_body has per pair: the A<->B image of window w is read across
// waves, and window w + 1 writes the exchange buffer again without the argmax's barriers in between.
//   out arrays and lag windows are indexed [(first_group + gl) * n_pairs + item.out].
// BS: empty, or one BandSet (the banded integrating instantiation, xspec_bands.hpp): gl is then an output ROW, group
// gl / n_bands under band gl % n_bands, and first_group the chunk's first row; the spectra are the group's real windows',
// and pair_body's 16-bit keep word zeroes the product -- built once when the band set is shared, rebuilt in front of
// every window's product when the bands are per window.
// CAF (the pack <LagBounds, Integrate, CafOperand>, integrate.hpp): operand j comes from spec_j, the de-rotated set; with
// caf_groups > 0 the launch holds every hypothesis and gl is a VIRTUAL group d * caf_groups + g -- operand j at virtual
// windows gl * K + kw, operand i and the lag interval at real group gl % caf_groups, the output slot virtual.  Otherwise
// spec_j and caf_groups are not read.
template <bool CAF = false, class... BS>
__device__ __forceinline__ void pair_body_integ(const float4* __restrict__ spec, const float4* spec_j, int caf_groups,
                                                const float4* __restrict__ tw1_g,
                                                const float2* __restrict__ tw2_g, const PairItem* __restrict__ items,
                                                const int* __restrict__ part_begin, int n_parts, int n_buoys, int n_pairs,
                                                int xcd_map, long first_group, float out_scale, int* __restrict__ lag_int,
                                                float* __restrict__ lag_frac, float* __restrict__ peak, LagBounds lb, int K,
                                                BS... bs_pack) {
    constexpr bool BANDED = sizeof...(BS) > 0;
    extern __shared__ __attribute__((aligned(16))) char smem_ig[];   // (pair_body's carve)
    float2* xl = reinterpret_cast<float2*>(smem_ig);
    float2* tw2_lds = reinterpret_cast<float2*>(smem_ig + kLdsXchg);
    float* red_max = reinterpret_cast<float*>(smem_ig + kLdsXchg + kLdsTw2);      // [8]
    int* red_k = reinterpret_cast<int*>(smem_ig + kLdsXchg + kLdsTw2 + 32);       // [1]
    float* red_tap = reinterpret_cast<float*>(smem_ig + kLdsXchg + kLdsTw2 + 48); // [3]

    const int t = threadIdx.x;
    const int p = t & 1, u = t >> 1;
    const int lane = t & 63, wave = t >> 6;
    int gl, part;   // (the placement of pair_body, with groups for windows)
    {
        const int b = blockIdx.x;
        if (xcd_map) {
            const int xcd = b & 7, s = b >> 3;
            gl = (s / n_parts) * 8 + xcd;
            part = s % n_parts;
        } else {
            gl = b / n_parts;
            part = b % n_parts;
        }
    }
    if (t < 256) tw2_lds[(t >> 4) * kTw2RowF2 + (t & 15)] = tw2_g[t];   // (load_tw2_to_lds)
    float2 tw1[16];   // resident over all windows and pairs (this instantiation has the registers: two waves per SIMD)
    load_tw1(tw1, tw1_g, t);
    __syncthreads();

    const float sgn = p ? -1.0f : 1.0f;
    const int kbase = p ? (u - 1) : (u + kM - 1);
    const int it_begin = part_begin[part];
    const int it_end = part_begin[part + 1];
    // banded: gl is a row (group gl / n_bands, band gl % n_bands); bit s of `keep` says whether this thread's slot s
    // lies in the band of the window about to be multiplied (role C: xspec_weight.hpp's k_fwd map)
    int gr = gl;
    [[maybe_unused]] int band_m = 0;
    [[maybe_unused]] unsigned keep = 0xffffu;
    [[maybe_unused]] auto keep_of = [&](int kw) -> unsigned {
        unsigned kp = 0xffffu;
        if constexpr (BANDED) {
            const BandSet bs = band_set_of(bs_pack...);
            const XBand bd = band_of_window(bs, (long)gr * K + kw, band_m);
            const int kb = RMX_XBIN_KFWD(p, u);
            kp = 0u;
#pragma unroll
            for (int s = 0; s < 16; ++s) kp |= (xband_keeps(bd, kb + kXbinKfwdSlot * s, kL - 1) ? 1u : 0u) << s;
        }
        return kp;
    };
    [[maybe_unused]] bool band_per_window = false;
    if constexpr (BANDED) {
        const BandSet bs = band_set_of(bs_pack...);
        gr = gl / bs.n_bands;
        band_m = gl - gr * bs.n_bands;
        band_per_window = bs.wstride != 0;
        keep = keep_of(0);
    }
    if constexpr (CAF) {   // the real group: operand i and the lag interval (gl stays the virtual one)
        if (caf_groups > 0) gr = gl % caf_groups;
    }
    const long gbase = (long)gr * K * n_buoys;   // item of the group's first window, buoy 0 (chunk-local)
    float4 sa[8], sb[8];   // X_i and X_j of the window about to be processed
    PairItem pi = items[it_begin < it_end ? it_begin : 0];
    auto request = [&](const PairItem& pr, int kw) {
        const float4* xi = spec + (gbase + (long)kw * n_buoys + pr.i) * (8 * kThreads);
        const float4* xj = spec + (gbase + (long)kw * n_buoys + pr.j) * (8 * kThreads);
        if constexpr (CAF)   // the (virtual) group's window kw in the de-rotated set
            xj = spec_j + (((long)gl * K + kw) * n_buoys + pr.j) * (8 * kThreads);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sa[j] = xi[j * kThreads + t];
            sb[j] = xj[j * kThreads + t];
        }
    };
    if (it_begin < it_end) request(pi, 0);
    for (int it = it_begin; it < it_end; ++it) {
        const int out_idx = pi.out;
        float acc[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
        for (int kw = 0; kw < K; ++kw) {
            float2 v[16];
#pragma unroll
            for (int j = 0; j < 8; ++j) {   // R = X_j * conj(X_i), (im, re)-swapped (pair_body)
                const float4 a = sa[j];
                const float4 b = sb[j];
                v[2 * j] = make_float2(b.y * a.x - b.x * a.y, b.x * a.x + b.y * a.y);
                v[2 * j + 1] = make_float2(b.w * a.z - b.z * a.w, b.z * a.z + b.w * a.w);
            }
            if constexpr (BANDED) {       // the band of THIS window: a dropped bin's product is +0
                if (band_per_window) keep = keep_of(kw);
#pragma unroll
                for (int s = 0; s < 16; ++s)
                    if (!((keep >> s) & 1u)) v[s] = make_float2(0.0f, 0.0f);
            }
            dft16(v);                     // k2 -> n0   (role C)
            mul_tw2(v, tw2_lds, u & 15);  // W_256^(k1*n0)
            xchg_bc_write_c(xl, v, t);
            wave_lds_fence();
            xchg_bc_read_b(xl, v, t);
            dft16(v);                     // k1 -> n1   (role B)
            xchg_b_write(xl, v, t);
            __syncthreads();
            xchg_a_read(xl, v, t);
            mul_tw1(v, tw1);              // W_M^(u*k0) [* W_L^u odd]
            dft16(v);                     // k0 -> n2   (role A)
            if (p) {
#pragma unroll
                for (int q = 1; q < 16; ++q) v[q] = cmul(v[q], w32(q));
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {   // last radix-2 stage across the lane pair, |.|^2, the running sum
                const float rx = sgn * v[q].x + dpp_xor1(v[q].x);
                const float ry = sgn * v[q].y + dpp_xor1(v[q].y);
                acc[q] += rx * rx + ry * ry;
            }
            if (kw + 1 < K) {
                request(pi, kw + 1);
            } else if (it + 1 < it_end) {
                pi = items[it + 1];
                request(pi, 0);
            }
            __syncthreads();   // every wave has read the A<->B image: the next window may write the exchange buffer
        }
        if (p && u == 0) acc[0] = -1.0f;   // lag -M is not part of 'full'
        int klo, khi;
        lag_window(lb, first_group + (CAF ? gr : gl), out_idx, kM - 1, klo, khi);
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = lag_mask(acc[q], kbase + q * 256, klo, khi);
        float tmax = acc[0];
#pragma unroll
        for (int q = 1; q < 16; ++q) tmax = fmaxf(tmax, acc[q]);
        float wmax = tmax;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, off, 64));
        if (lane == 0) red_max[wave] = wmax;
        if (t == 0) *red_k = 0x7fffffff;
        __syncthreads();
        float gmax = red_max[0];
#pragma unroll
        for (int w = 1; w < 8; ++w) gmax = fmaxf(gmax, red_max[w]);
        if (tmax == gmax) {
            int kmin = 0x7fffffff;
#pragma unroll
            for (int q = 15; q >= 0; --q)
                if (acc[q] == gmax) kmin = kbase + q * 256;
            atomicMin(red_k, kmin);
        }
        __syncthreads();
        const int kstar = *red_k;
#pragma unroll
        for (int d = -1; d <= 1; ++d) {   // owners of taps k*-1, k*, k*+1 publish sqrt(sum) (scipy scaling)
            const int kk = kstar + d;
            if (kk >= 0 && kk <= 2 * kM - 2) {
                const int par = (kk >= kM - 1) ? 0 : 1;
                const int n = par ? (kk + 1) : (kk - (kM - 1));
                if (p == par && u == (n & 255)) {
                    const int qo = n >> 8;
                    float val = 0.0f;
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (q == qo) val = acc[q];
                    red_tap[d + 1] = sqrtf(val) * out_scale;
                }
            }
        }
        __syncthreads();
        if (t == 0) {
            const double b = (double)red_tap[1];
            double frac = 0.0;
            if (kstar > klo && kstar < khi) {
                const double a = (double)red_tap[0], c = (double)red_tap[2];
                const double den = a - 2.0 * b + c;
                if (den != 0.0) frac = 0.5 * (a - c) / den;
            }
            const long o = (first_group + gl) * (long)n_pairs + out_idx;
            lag_int[o] = kstar - (kM - 1);
            lag_frac[o] = (float)frac;
            peak[o] = (float)b;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Resident pair kernel (one workgroup per CU, <= 256 VGPRs).  One workgroup barrier per pair:
//   pair n:  product -> [request X_j of pair n+1] -> DFT16 -> TW2 -> wave-local exchange -> DFT16 ->
//            write A<->B image -> BARRIER -> [resolve pair n-1] -> read image -> TW1 -> DFT16 -> W32 ->
//            lane-pair butterfly, |.|^2 -> publish: all |.|^2 to an LDS tap buffer, wave winner
//            (max, lowest 'full' index) to an LDS slot.
// The cross-wave part of the argmax and the 3-tap parabola of pair n are "resolved" by one lane
// after the barrier of pair n+1 (both LDS buffers are double buffered by pair parity), so the
// reduction's latency chain hides behind the next pair's arithmetic.
constexpr int kLdsMag = kL * 4;                         // one |.|^2 image: [q4][t] float4
constexpr int kLdsResOff = kLdsXchg + kLdsTw2;
constexpr int kLdsResBytes = kLdsXchg + kLdsTw2 + 2 * kLdsMag + 256;

template <bool BOUNDED>
__device__ __forceinline__ void resolve_pair(const float* magbuf, const float2* red, long out_pos, float out_scale,
                                             int* __restrict__ lag_int, float* __restrict__ lag_frac,
                                             float* __restrict__ peak, LagBounds lb, long w, int q_out) {
    // red[w] = (wave max of |r|^2 as float bits, lowest 'full' index attaining it), w = 0..7
    float gmax = -2.0f;
    int kstar = 0x7fffffff;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const float2 e = red[w];
        const float m = e.x;
        const float ey = e.y;
        const int k = __builtin_bit_cast(int, ey);
        if (m > gmax || (m == gmax && k < kstar)) { gmax = m; kstar = k; }
    }
    auto tap = [&](int kk) -> float {
        const int par = (kk >= kM - 1) ? 0 : 1;
        const int n = par ? (kk + 1) : (kk - (kM - 1));
        const int tt = 2 * (n & 255) + par, q = n >> 8;
        return sqrtf(magbuf[((q >> 2) * kThreads + tt) * 4 + (q & 3)]) * out_scale;
    };
    const float b = sqrtf(gmax) * out_scale;
    float frac = 0.0f;
    int klo = 0, khi = 2 * kM - 2;
    if constexpr (BOUNDED) lag_window(lb, w, q_out, kM - 1, klo, khi);
    if (kstar > klo && kstar < khi) {
        const float a = tap(kstar - 1), c = tap(kstar + 1);
        const double den = (double)a - 2.0 * (double)b + (double)c;
        if (den != 0.0) frac = (float)(0.5 * ((double)a - (double)c) / den);
    }
    lag_int[out_pos] = kstar - (kM - 1);
    lag_frac[out_pos] = frac;
    peak[out_pos] = b;
}

// LB: empty, one LagBounds (the bounded instantiation), or <BandSet> / <LagBounds, BandSet> (the banded ones, xspec_bands.hpp)
template <class... LB>
__global__ __launch_bounds__(kThreads, 2) void k_pair_res(
    const float4* __restrict__ spec, const float4* __restrict__ spec_j, const float4* __restrict__ tw1_g, const float2* __restrict__ tw2_g,
    const PairItem* __restrict__ items, const int* __restrict__ part_begin, int n_parts, int n_buoys, int n_pairs,
    int xcd_map, long first_window, float out_scale, int* __restrict__ lag_int, float* __restrict__ lag_frac,
    float* __restrict__ peak, int /* was dbg_rt */, int i_wrap, LB... lb_pack) {
    constexpr bool BOUNDED = kHasBounds<LB...>, BANDED = kBanded<LB...>;
    const LagBounds lb = lag_bounds_of(lb_pack...);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* xl = reinterpret_cast<float2*>(smem);
    float2* tw2_lds = reinterpret_cast<float2*>(smem + kLdsXchg);
    float4* magbuf = reinterpret_cast<float4*>(smem + kLdsResOff);                 // [2][4][512] float4
    float2* red = reinterpret_cast<float2*>(smem + kLdsResOff + 2 * kLdsMag);      // [2][8]

    const int t = threadIdx.x;
    const int p = t & 1, u = t >> 1;
    const int lane = t & 63, wave = t >> 6;
    int wl, part;
    {
        const int b = blockIdx.x;
        if (xcd_map) {
            const int xcd = b & 7, s = b >> 3;
            wl = (s / n_parts) * 8 + xcd;
            part = s % n_parts;
        } else {
            wl = b / n_parts;
            part = b % n_parts;
        }
    }
    load_tw2_to_lds(tw2_lds, tw2_g, t);
    float2 tw1[16];
    load_tw1(tw1, tw1_g, t);
    __syncthreads();

    const float sgn = p ? -1.0f : 1.0f;
    const int kbase = p ? (u - 1) : (u + kM - 1);
    const int it_begin = part_begin[part];
    const int it_end = part_begin[part + 1];
    if (it_begin >= it_end) return;
    // banded: wl is a VIRTUAL window (real window wl / n_bands, band wl % n_bands); both spectra are the real window's,
    // and bit s of `keep` says whether this thread's slot s lies in the band (role C: xspec_weight.hpp's k_fwd map)
    // (rmx_caf_batch_bands, all hypotheses in one launch: i_wrap in virtual windows, as pair_body)
    int wr = wl;
    [[maybe_unused]] int wr_i = wl;
    [[maybe_unused]] unsigned keep = 0xffffu;
    if constexpr (BANDED) {
        const BandSet bs = band_set_of(lb_pack...);
        const int vi = i_wrap > 0 ? wl % i_wrap : wl;
        wr = band_real_window(bs, wl);
        wr_i = band_real_window(bs, vi);
        const XBand bd = band_of_virtual(bs, vi);
        const int kb = RMX_XBIN_KFWD(p, u);
        keep = 0u;
#pragma unroll
        for (int s = 0; s < 16; ++s) keep |= (xband_keeps(bd, kb + kXbinKfwdSlot * s, kL - 1) ? 1u : 0u) << s;
    }
    const long wbase = (long)wr * n_buoys;
    long wbase_i;
    if constexpr (BANDED) wbase_i = (long)wr_i * n_buoys;
    else wbase_i = (long)(i_wrap > 0 ? wl % i_wrap : wr) * n_buoys;   // (rmx_caf_batch: wl = hypothesis * windows + window)
    const long obase = (first_window + wl) * (long)n_pairs;
    // the window whose lag bounds apply (one launch for all hypotheses: the REAL window; the output slot stays virtual)
    [[maybe_unused]] const long lbw = first_window + (i_wrap > 0 ? wl % i_wrap : wl);
    float4 sa[8], sb[8];
    PairItem pi = items[it_begin];
    int cur_i = pi.i;
    {
        const float4* xi = spec + (wbase_i + pi.i) * (8 * kThreads);
        const float4* xj = spec_j + (wbase + pi.j) * (8 * kThreads);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sa[j] = xi[j * kThreads + t];
            sb[j] = xj[j * kThreads + t];
        }
    }
    int prev_out = -1;
    for (int it = it_begin; it < it_end; ++it) {
        const int out_idx = pi.out;
        const int buf = (it - it_begin) & 1;
        float2 v[16];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 a = sa[j];
            const float4 b = sb[j];
            v[2 * j] = make_float2(b.y * a.x - b.x * a.y, b.x * a.x + b.y * a.y);
            v[2 * j + 1] = make_float2(b.w * a.z - b.z * a.w, b.z * a.z + b.w * a.w);
        }
        if constexpr (BANDED) {   // the band: a dropped bin's product is +0
#pragma unroll
            for (int s = 0; s < 16; ++s)
                if (!((keep >> s) & 1u)) v[s] = make_float2(0.0f, 0.0f);
        }
        if (it + 1 < it_end) {   // request the next pair's spectra: a whole pair of compute hides it
            pi = items[it + 1];
            const float4* xj = spec_j + (wbase + pi.j) * (8 * kThreads);
#pragma unroll
            for (int j = 0; j < 8; ++j) sb[j] = xj[j * kThreads + t];
            if (pi.i != cur_i) {
                cur_i = pi.i;
                const float4* xi = spec + (wbase_i + pi.i) * (8 * kThreads);
#pragma unroll
                for (int j = 0; j < 8; ++j) sa[j] = xi[j * kThreads + t];
            }
        }
        dft16(v);                     // k2 -> n0   (role C)
        mul_tw2(v, tw2_lds, u & 15);  // W_256^(k1*n0)
        xchg_bc_write_c(xl, v, t);
        wave_lds_fence();
        xchg_bc_read_b(xl, v, t);
        dft16(v);                     // k1 -> n1   (role B)
        xchg_b_write(xl, v, t);       // into this half wave's own region
        __syncthreads();              // the pair's only barrier; also publishes pair it-1's winners
        if (prev_out >= 0 && t == ((it - it_begin) & 7) * 64)
            resolve_pair<BOUNDED>(reinterpret_cast<const float*>(magbuf + (buf ^ 1) * (4 * kThreads)), red + (buf ^ 1) * 8,
                                  obase + prev_out, out_scale, lag_int, lag_frac, peak, lb, lbw, prev_out);
        xchg_a_read(xl, v, t);
        mul_tw1(v, tw1);              // W_M^(u*k0) [* W_L^u on odd lanes]
        dft16(v);                     // k0 -> n2   (role A): e[n] (even lanes) / o[n]*W_L^u (odd lanes)
        if (p) {
#pragma unroll
            for (int q = 1; q < 16; ++q) v[q] = cmul(v[q], w32(q));
        }
        float mag[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float rx = sgn * v[q].x + dpp_xor1(v[q].x);
            const float ry = sgn * v[q].y + dpp_xor1(v[q].y);
            mag[q] = rx * rx + ry * ry;
        }
        if (p && u == 0) mag[0] = -1.0f;   // lag -M is not part of the 'full' output
        if constexpr (BOUNDED) {           // lag window: |r|^2 outside it -> the same sentinel (lag_bounds.hpp)
            int klo, khi;
            lag_window(lb, lbw, out_idx, kM - 1, klo, khi);
#pragma unroll
            for (int q = 0; q < 16; ++q) mag[q] = lag_mask(mag[q], kbase + q * 256, klo, khi);
        }
        float4* mb = magbuf + buf * (4 * kThreads) + t;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
            mb[q4 * kThreads] = make_float4(mag[4 * q4], mag[4 * q4 + 1], mag[4 * q4 + 2], mag[4 * q4 + 3]);
        float tmax = mag[0];
#pragma unroll
        for (int q = 1; q < 16; ++q) tmax = fmaxf(tmax, mag[q]);
        int kq = 0;
#pragma unroll
        for (int q = 15; q >= 0; --q)
            if (mag[q] == tmax) kq = kbase + q * 256;   // lowest 'full' index of this lane's maximum
        const float wmax = wave_max_f32(tmax);
        const int kw = wave_min_i32(tmax == wmax ? kq : 0x7fffffff);
        if (lane == 0) red[buf * 8 + wave] = make_float2(wmax, __builtin_bit_cast(float, kw));
        prev_out = out_idx;
    }
    __syncthreads();
    if (t == 0) {
        const int buf = (it_end - 1 - it_begin) & 1;
        resolve_pair<BOUNDED>(reinterpret_cast<const float*>(magbuf + buf * (4 * kThreads)), red + buf * 8, obase + prev_out,
                              out_scale, lag_int, lag_frac, peak, lb, lbw, prev_out);
    }
}

#define RMX_PAIR_ARGS                                                                                         \
    const float4 *__restrict__ spec, const float4 *__restrict__ spec_j, const float4 *__restrict__ tw1_g,     \
        const float2 *__restrict__ tw2_g,                                                                     \
        const PairItem *__restrict__ items, const int *__restrict__ part_begin, int n_parts, int n_buoys,     \
        int n_pairs, int xcd_map, long first_window, float out_scale, int *__restrict__ lag_int,              \
        float *__restrict__ lag_frac, float *__restrict__ peak, int i_wrap
#define RMX_PAIR_PASS                                                                                         \
    spec, spec_j, tw1_g, tw2_g, items, part_begin, n_parts, n_buoys, n_pairs, xcd_map, first_window, out_scale,      \
        lag_int, lag_frac, peak, i_wrap

// LB: empty, one LagBounds (the bounded instantiation), <LagBounds, Integrate> (the integrating one, integrate.hpp:
// first_window is then the chunk's first GROUP; spec_j and i_wrap are not used), <LagBounds, Integrate, CafOperand> (the
// integrated Doppler search's: operand j from spec_j), <BandSet> / <LagBounds, BandSet> (the
// banded ones, xspec_bands.hpp: first_window is then the chunk's first VIRTUAL window), or <LagBounds, Integrate, BandSet>
// (the banded integrating one: first_window is the chunk's first ROW, group * n_bands + band)
template <class... LB>
__global__ __launch_bounds__(kThreads, kIntegrating<LB...> ? 2 : 4) void k_pair_str(RMX_PAIR_ARGS, LB... lb) {
    if constexpr (kIntegrating<LB...> && kBanded<LB...>) {
        pair_body_integ(spec, spec, 0, tw1_g, tw2_g, items, part_begin, n_parts, n_buoys, n_pairs, xcd_map, first_window, out_scale,
                        lag_int, lag_frac, peak, integ_bounds(lb...), integ_windows(lb...), band_set_of(lb...));
    } else if constexpr (kCafOperand<LB...>) {   // (first_window: the chunk's first GROUP; i_wrap is not used)
        pair_body_integ<true>(spec, spec_j, caf_groups(lb...), tw1_g, tw2_g, items, part_begin, n_parts, n_buoys, n_pairs, xcd_map,
                              first_window, out_scale, lag_int, lag_frac, peak, integ_bounds(lb...), integ_windows(lb...));
    } else if constexpr (kIntegrating<LB...>) {
        pair_body_integ(spec, spec, 0, tw1_g, tw2_g, items, part_begin, n_parts, n_buoys, n_pairs, xcd_map, first_window, out_scale,
                        lag_int, lag_frac, peak, integ_bounds(lb...), integ_windows(lb...));
    } else if constexpr (kBanded<LB...>) {
        pair_body<kHasBounds<LB...>>(RMX_PAIR_PASS, lag_bounds_of(lb...), band_set_of(lb...));
    } else {
        pair_body<(sizeof...(LB) > 0)>(RMX_PAIR_PASS, lag_bounds_of(lb...));
    }
}

}  // namespace rmx
