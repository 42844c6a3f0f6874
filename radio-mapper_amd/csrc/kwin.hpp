// kwin.hpp -- the fused window kernel of the tuned N = 4096 path (k_win), its peak-record resolve routine, the
// table loaders it shares with k_fwd / the pair kernels, and the host-side builder of its twiddle tables.
// A header of its own so that tools/probe/kwin_bench.hip can compile and time this kernel on its own; rmx_hip.hip
// includes it unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>
#include <vector>

#include "fft_r16.hpp"
#include "lag_bounds.hpp"

namespace rmx {

using u32x4 = unsigned int __attribute__((ext_vector_type(4)));
using u32x2 = unsigned int __attribute__((ext_vector_type(2)));
using f32x4 = float __attribute__((ext_vector_type(4)));
using f32x2 = float __attribute__((ext_vector_type(2)));
// NOTE: __builtin_bit_cast(float, vec.y) on a vector ELEMENT is mis-lowered by this hipcc (every
// element reads lane 0 of the vector); always bit_cast the whole vector, then take elements.

// LDS carve (bytes) of both kernels: exchange image, TW2 table, reduction words
constexpr int kLdsXchg = kXchgF2 * 8;                  // 69632
constexpr int kLdsTw2 = 16 * kTw2RowF2 * 8;            // 2304
constexpr int kLdsRed = 64;
constexpr int kLdsBytes = kLdsXchg + kLdsTw2 + kLdsRed;

__device__ __forceinline__ void load_tw2_to_lds(float2* tw2_lds, const float2* __restrict__ tw2_g, int t) {
    // tw2_g: [16][16] complex; LDS rows padded to kTw2RowF2
    if (t < 256) tw2_lds[(t >> 4) * kTw2RowF2 + (t & 15)] = tw2_g[t];
}

// same table in layer-1 group order for dft16_tw_row: stored[4*q0 + m - 1] = tw2[a][q0 + 4*m]; the
// unused tw2[a][0] = 1 goes to the pad slot 15
__device__ __forceinline__ void load_tw2_to_lds_grouped(float2* tw2_lds, const float2* __restrict__ tw2_g, int t) {
    if (t < 256) {
        const int a = t >> 4, q = t & 15;
        tw2_lds[a * kTw2RowF2 + (q == 0 ? 15 : 4 * (q & 3) + (q >> 2) - 1)] = tw2_g[t];
    }
}

__device__ __forceinline__ void load_tw1(float2 (&tw1)[16], const float4* __restrict__ tw1_g, int t) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float4 w = tw1_g[j * kThreads + t];
        tw1[2 * j] = make_float2(w.x, w.y);
        tw1[2 * j + 1] = make_float2(w.z, w.w);
    }
}

// ------------------------------------------------------------------------------------------------
// Fused window kernel: one workgroup (512 threads, <= 256 VGPRs, one per CU) per capture window.
//   phase 1  forward spectra of all B buoys -> this window's scratch (thread-private layout: every
//            thread later re-reads exactly the float4s it stored, so no visibility protocol is needed)
//   phase 2  the remaining pairs in runs that hand the anchor over: consecutive pairs share a spectrum that stays in
//            registers, the other one streams one pair ahead; conj-multiply merged into the first radix-16 pass; ONE workgroup barrier per pair.
// LDS: two exchange images (alternating by transform/pair, which is what makes one barrier enough:
// a wave only writes its own half-wave regions of the image the others are not reading), the TW2
// table, and two small double-buffered records per wave for the argmax: the wave's winner with its
// in-wave neighbour taps, and a "halo" of the |r|^2 of its lanes 0,1,62,63 for neighbours that sit
// in another wave.  The pair's winner is resolved by one lane after the NEXT pair's barrier.
constexpr int kLdsWinImg = kLdsXchg;                                 // 69632 each, two of them
constexpr int kLdsWinTw2 = 2 * kLdsWinImg;
constexpr int kResWaveMask = 7;   // the resolving wave rotates over all eight waves (seq & 7)
constexpr int kResSlots = 8;   // record ring; winners are resolved in batches of kResBatch pairs
constexpr int kResBatch = 7;   // < kResSlots: the pair after a batch writes a slot the resolver is not reading
constexpr int kHaloRows = 4;
constexpr int kLdsWinHalo = kLdsWinTw2 + kLdsTw2;                           // [slots][8][rows][16] float
constexpr int kLdsWinRed = kLdsWinHalo + kResSlots * 8 * kHaloRows * 16 * 4;   // [slots][8] float4
constexpr int kLdsWinOidx = kLdsWinRed + kResSlots * 8 * 16;                // [slots] int: output slot of the pair
constexpr int kLdsWinBytes = kLdsWinOidx + kResSlots * 4;
static_assert(kLdsWinBytes <= 160 * 1024, "k_win LDS");

__device__ __forceinline__ void k_to_owner(int kk, int& tt, int& q) {
    const int par = (kk >= kM - 1) ? 0 : 1;
    const int n = par ? (kk + 1) : (kk - (kM - 1));
    tt = 2 * (n & 255) + par;
    q = n >> 8;
}

// Executed by ONE whole wave after a barrier that published the records of `cnt` <= 7 pairs (ring
// slots first, first+1, ...): lane = 8*g + r looks at wave r's record of the g-th pair, two DPP
// reductions over each group of 8 lanes pick (max |r|^2, lowest 'full' index), the neighbour taps
// come from the winner's own record or from the halo rows, and the winning lane of every group
// stores the pair's 12 bytes.  One resolve per 7 pairs instead of one per pair: the resolving wave
// is late to its next barrier by the length of this routine, and the other seven wait for it.
// BOUNDED: frac = 0 at the edges of the pair's lag window (lag_bounds.hpp), window w (global index)
template <bool BOUNDED = false>
__device__ __forceinline__ void resolve_batch(int lane, const float4* red, const float* halo, const int* oidx,
                                              int first, int cnt, long obase, float out_scale,
                                              int* __restrict__ lag_int, float* __restrict__ lag_frac,
                                              float* __restrict__ peak, LagBounds lb = {}, long w = 0) {
    const int g = lane >> 3, r = lane & 7;
    const bool act = g < cnt;
    const int slot = (first + g) & (kResSlots - 1);
    // record = {max |r|^2, its lowest 'full' index (int bits), tap k*-1, tap k*+1}; scalar LDS reads
    const float* rf = reinterpret_cast<const float*>(red) + 4 * (slot * 8 + r);
    const int* ri = reinterpret_cast<const int*>(rf);
    const float ex = act ? rf[0] : -3.0f;
    const int k = act ? ri[1] : 0x7fffffff;
    const float tm = rf[2], tp = rf[3];
    const int out = oidx[slot];
    float gmax = ex;                                     // max over the 8 lanes of the group
    gmax = fmaxf(gmax, __builtin_bit_cast(float, dpp_i<0xB1>(__builtin_bit_cast(int, gmax))));
    gmax = fmaxf(gmax, __builtin_bit_cast(float, dpp_i<0x4E>(__builtin_bit_cast(int, gmax))));
    gmax = fmaxf(gmax, __builtin_bit_cast(float, dpp_i<0x141>(__builtin_bit_cast(int, gmax))));
    int kstar = (ex == gmax) ? k : 0x7fffffff;
    kstar = min(kstar, dpp_i<0xB1>(kstar));
    kstar = min(kstar, dpp_i<0x4E>(kstar));
    kstar = min(kstar, dpp_i<0x141>(kstar));
    const bool win = act && ex == gmax && k == kstar;     // exactly one lane per active group
    // halo rows (always read, clamped): only lanes 0,1,62,63 of a wave can own a cross-wave neighbour
    auto halo_tap = [&](int kk) -> float {
        kk = kk < 0 ? 0 : (kk > 2 * kM - 2 ? 2 * kM - 2 : kk);
        int tt, q;
        k_to_owner(kk, tt, q);
        const int ln = tt & 63;
        const int row = ln < 2 ? ln : (ln >= 62 ? ln - 60 : 0);
        return halo[(((slot * 8 + (tt >> 6)) * kHaloRows) + row) * 16 + q];
    };
    const int kc = win ? k : (kM - 1);
    const float hm = halo_tap(kc - 1), hp = halo_tap(kc + 1);
    const float b = sqrtf(fmaxf(ex, 0.0f)) * out_scale;
    const float a = sqrtf(tm >= 0.0f ? tm : hm) * out_scale;
    const float c = sqrtf(tp >= 0.0f ? tp : hp) * out_scale;
    const double den = (double)a - 2.0 * (double)b + (double)c;
    float frac = 0.0f;
    if constexpr (BOUNDED) {
        int klo = 0, khi = 0;
        if (act) lag_window(lb, w, out, kM - 1, klo, khi);
        if (kc > klo && kc < khi && den != 0.0) frac = (float)(0.5 * ((double)a - (double)c) / den);
    } else {
        if (kc > 0 && kc < 2 * kM - 2 && den != 0.0) frac = (float)(0.5 * ((double)a - (double)c) / den);
    }
    if (win) {
        lag_int[obase + out] = kc - (kM - 1);
        lag_frac[obase + out] = frac;
        peak[obase + out] = b;
    }
}

// Schedule of one window (all pairs i<j of B buoys; two register arrays of one spectrum each, sa and sb):
//   anchor 0      X_0 is transformed straight into sa (never stored); every further X_e is transformed once into sb,
//                 stored once, and used at once, from registers, for (0,e).  X_{B-1} stays in sb behind this phase and is
//                 not stored either: the table never requests it (host::trail_kernel_ok) and the scratch is private to
//                 the workgroup, so its slot of the scratch stays unwritten;
//   handover runs the pairs among buoys 1 .. B-1 in the order of a host-planned table (host::plan_pair_trail, `trail`).
//                 A run keeps its anchor in one array and streams its partners through the other, one pair ahead; the
//                 partner streamed last stays where it is as the next run's anchor, and the stream moves to the array the
//                 old anchor leaves.  Anchors go B-1, 1, B-2, 2, ..., each with the buoys that have not been anchor yet,
//                 each run walking the previous run's order backwards.  Every step requests ONE spectrum; no anchor is
//                 ever loaded and no step loads both arrays, whatever the parity or size of B.  X_i is in sa and X_j in
//                 sb at every step, as the anchor runs had them, so every pair's arithmetic is what it was; the request
//                 goes to sa or to sb (two copies of h1).
// Requests per window at B = 8: 8 inputs (256 KiB) + 6 spectrum stores (384 KiB: X_1 .. X_6) + 21 spectrum loads of 64 KiB
// (one from the last pair of anchor 0, 20 from the table's steps; a 22nd, behind the last step, goes into dead registers).
template <bool U8>
__global__ __launch_bounds__(kThreads, 2) void k_win(const void* __restrict__ iq_v, float4* __restrict__ spec,
                                                     const float4* __restrict__ tw1_g,
                                                     const float2* __restrict__ tw2_g, int n_buoys,
                                                     long first_window, float out_scale,
                                                     int* __restrict__ lag_int, float* __restrict__ lag_frac,
                                                     float* __restrict__ peak, int n_win, const int4* __restrict__ trail, int stag) {
    constexpr bool BOUNDED = false;
    constexpr LagBounds lb{nullptr, 0, 0, 0};   // (named by the bounded branches only)
#include "kwin_body.hpp"
}

// k_win with the caller's lag window per pair (rmx_xcorr_batch_bounded): the same body, BOUNDED = true.  A kernel of its
// own name rather than a third template argument, so that k_win keeps exactly its two instantiations.
template <bool U8>
__global__ __launch_bounds__(kThreads, 2) void k_win_lb(const void* __restrict__ iq_v, float4* __restrict__ spec,
                                                        const float4* __restrict__ tw1_g,
                                                        const float2* __restrict__ tw2_g, int n_buoys,
                                                        long first_window, float out_scale,
                                                        int* __restrict__ lag_int, float* __restrict__ lag_frac,
                                                        float* __restrict__ peak, int n_win, const int4* __restrict__ trail, int stag, LagBounds lb) {
    constexpr bool BOUNDED = true;
#include "kwin_body.hpp"
}

// ---- host: twiddle tables of k_fwd / k_win / the pair kernels ---------------------------------------
constexpr int kTw1ScaleLog2 = 6;                       // spectra carry 2^-6 (L = 2^13: sqrt(L) rounded down)
constexpr double kTw1Scale = 1.0 / (1 << kTw1ScaleLog2);
inline void build_tables(std::vector<float4>& tw1, std::vector<float2>& tw2) {
    const double two_pi = 6.283185307179586476925286766559;
    tw1.resize(8 * kThreads);
    std::vector<float2> t1(16 * kThreads);
    for (int t = 0; t < kThreads; ++t) {
        const int p = t & 1, u = t >> 1;
        for (int k0 = 0; k0 < 16; ++k0) {
            // W_M^(u*k0) * (p ? W_L^u : 1), W_n = exp(-2*pi*i/n)
            double ang = -two_pi * (double)((u * k0) % kM) / (double)kM;
            if (p) ang += -two_pi * (double)u / (double)kL;
            // the power-of-two scale of the forward spectra rides on this table (exact): the forward
            // transform multiplies by it once, the inverse once more (undone in out_scale)
            t1[k0 * kThreads + t] = make_float2((float)(std::cos(ang) * kTw1Scale), (float)(std::sin(ang) * kTw1Scale));
        }
    }
    for (int j = 0; j < 8; ++j)
        for (int t = 0; t < kThreads; ++t) {
            const float2 a = t1[(2 * j) * kThreads + t], b = t1[(2 * j + 1) * kThreads + t];
            tw1[j * kThreads + t] = make_float4(a.x, a.y, b.x, b.y);
        }
    tw2.resize(256);
    for (int a = 0; a < 16; ++a)
        for (int b = 0; b < 16; ++b) {
            const double ang = -two_pi * (double)((a * b) % 256) / 256.0;
            tw2[a * 16 + b] = make_float2((float)std::cos(ang), (float)std::sin(ang));
        }
}

}  // namespace rmx
