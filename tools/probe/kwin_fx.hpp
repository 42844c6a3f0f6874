// kwin_fx.hpp -- PROBE kernel for the forward transform's barrier exchange (LABNOTES R17) in tools/probe/kwin_bench.hip:
// k_win's body as it stood before R17 (kwin_fx_body.hpp, a copy of radio-mapper_amd/csrc/kwin_body.hpp) with the levers
// below behind the bits of FX.  Never part of the library.  FX = 0 compiles to the instruction body of that k_win.
//   1   lever A: the sixteen role-B reads of fwd are sixteen ds_read_b64 of ONE asm statement, in layer-1 consumption
//       order, waited for at its end (the compiler pairs the C++ reads into eight ds_read2_b64, 8 array cycles each
//       against 2 x 2)
//   2   lever B: fwd exchanges through a forward-only image [k0][n1][n0 >> 3][p][n0 & 7] (role A's ds_write_b64 conflict
//       free; the inverse transforms keep [k0][n1][p][n0])
//   4   the sixteen role-B stores of pair_h1 as sixteen ds_write_b64 (four per asm statement) instead of the eight
//       ds_write2st64_b64 / ds_write2_b64 the compiler makes of them
//   8   with 1: the values read are made opaque scalars (without it the register pairs the reads land in draw
//       v_pk_add_f32 into the first butterfly layer behind them; the sums are the same bits either way)
//   16  with 2: the two bases of the forward image are computed from the thread index at every transform instead of being
//       held in registers for the launch (219 VGPRs, the count before R17, instead of 223)
//   32  with 2: the same, derived from the inverse image's bases, which are live anyway (221 VGPRs)
// What shipped is FX = 3; the harness's k_win is that kernel, `fx 0` the one before it.
#pragma once
#include "../../radio-mapper_amd/csrc/kwin.hpp"

namespace rmx {

// (the forward-only image's index functions xa2f_base / xb2f_base are those of fft_r16.hpp)

// role B's sixteen slots (n1 = 0..15, 256 bytes apart) from LDS byte address `addr`, as sixteen ds_read_b64 in the order
// layer 1 of dft16 consumes them.  ONE statement that waits for its own reads: the compiler does not count LDS
// instructions it cannot see, so nothing may leave the statement in flight.
__device__ __forceinline__ void xchg_b2_read_plain(int addr, float2 (&v)[16]) {
    f32x2 r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15;
    asm volatile(
        "ds_read_b64 %0, %16\n\tds_read_b64 %4, %16 offset:1024\n\t"
        "ds_read_b64 %8, %16 offset:2048\n\tds_read_b64 %12, %16 offset:3072\n\t"
        "ds_read_b64 %1, %16 offset:256\n\tds_read_b64 %5, %16 offset:1280\n\t"
        "ds_read_b64 %9, %16 offset:2304\n\tds_read_b64 %13, %16 offset:3328\n\t"
        "ds_read_b64 %2, %16 offset:512\n\tds_read_b64 %6, %16 offset:1536\n\t"
        "ds_read_b64 %10, %16 offset:2560\n\tds_read_b64 %14, %16 offset:3584\n\t"
        "ds_read_b64 %3, %16 offset:768\n\tds_read_b64 %7, %16 offset:1792\n\t"
        "ds_read_b64 %11, %16 offset:2816\n\tds_read_b64 %15, %16 offset:3840\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7), "=&v"(r8), "=&v"(r9),
          "=&v"(r10), "=&v"(r11), "=&v"(r12), "=&v"(r13), "=&v"(r14), "=&v"(r15)
        : "v"(addr)
        : "memory");
#define RMX_FX_OUT(q) v[q] = make_float2(r##q.x, r##q.y);
    RMX_FX_OUT(0) RMX_FX_OUT(1) RMX_FX_OUT(2) RMX_FX_OUT(3) RMX_FX_OUT(4) RMX_FX_OUT(5) RMX_FX_OUT(6) RMX_FX_OUT(7)
    RMX_FX_OUT(8) RMX_FX_OUT(9) RMX_FX_OUT(10) RMX_FX_OUT(11) RMX_FX_OUT(12) RMX_FX_OUT(13) RMX_FX_OUT(14) RMX_FX_OUT(15)
#undef RMX_FX_OUT
}

// four role-B stores (slots S, S+4, S+8, S+12 of the k0 row at LDS byte address `addr`) as four ds_write_b64
template <int S>
__device__ __forceinline__ void xchg_b2_write4_plain(int addr, const float2& a, const float2& b, const float2& c, const float2& d) {
    const f32x2 va = {a.x, a.y}, vb = {b.x, b.y}, vc = {c.x, c.y}, vd = {d.x, d.y};
    asm volatile("ds_write_b64 %0, %1 offset:%5\n\tds_write_b64 %0, %2 offset:%6\n\t"
                 "ds_write_b64 %0, %3 offset:%7\n\tds_write_b64 %0, %4 offset:%8"
                 ::"v"(addr), "v"(va), "v"(vb), "v"(vc), "v"(vd), "n"(S * 256), "n"((S + 4) * 256), "n"((S + 8) * 256),
                   "n"((S + 12) * 256)
                 : "memory");
}

template <bool U8, int FX>
__global__ __launch_bounds__(kThreads, 2) void k_win_fx(const void* __restrict__ iq_v, float4* __restrict__ spec,
                                                        const float4* __restrict__ tw1_g,
                                                        const float2* __restrict__ tw2_g, int n_buoys,
                                                        long first_window, float out_scale,
                                                        int* __restrict__ lag_int, float* __restrict__ lag_frac,
                                                        float* __restrict__ peak, int n_win, const int4* __restrict__ trail, int stag) {
    constexpr bool BOUNDED = false;
    constexpr LagBounds lb{nullptr, 0, 0, 0};
#include "kwin_fx_body.hpp"
}

}  // namespace rmx
