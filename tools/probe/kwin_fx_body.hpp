// kwin_fx_body.hpp -- PROBE copy of radio-mapper_amd/csrc/kwin_body.hpp as it stood before LABNOTES R17, included by
// kwin_fx.hpp into k_win_fx; the levers of the forward exchange hang on the bits of FX (see there).
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* img0 = reinterpret_cast<float2*>(smem);
    float2* img1 = reinterpret_cast<float2*>(smem + kLdsWinImg);
    float2* tw2_lds = reinterpret_cast<float2*>(smem + kLdsWinTw2);
    float* halo = reinterpret_cast<float*>(smem + kLdsWinHalo);
    float4* red = reinterpret_cast<float4*>(smem + kLdsWinRed);
    int* oidx = reinterpret_cast<int*>(smem + kLdsWinOidx);

    const int t = threadIdx.x;
    const int p = t & 1, u = t >> 1;
    const int lane = t & 63, wave = t >> 6;
    const int B = n_buoys;
    const int n_pairs = B * (B - 1) / 2;

    load_tw2_to_lds_grouped(tw2_lds, tw2_g, t);
    float2 tw1[16];
    load_tw1(tw1, tw1_g, t);
    // second-generation exchanges (fft_r16.hpp): roles B and C keep their own digit (n0 / k1) in lane bits 0-3
    const float4* tw2row = reinterpret_cast<const float4*>(tw2_lds + (t & 15) * kTw2RowF2);
    const int loc_m0[2] = {__builtin_amdgcn_readfirstlane(wave * kLocWave),                 // this wave's region of image 0 / 1
                           __builtin_amdgcn_readfirstlane(kLdsWinImg + wave * kLocWave)};
    const int loc_rd = wave * kLocWave + loc_read_off(lane);
    const float sgn = p ? -1.0f : 1.0f;
    const int kbase = p ? (u - 1) : (u + kM - 1);
    const int hl = lane < 2 ? lane : lane - 60;            // halo row of lanes 0,1,62,63
    const bool is_halo = lane < 2 || lane >= 62;
    __syncthreads();
    // this thread's TW2 row W_256^(n0*k1), k1 = 0..15, kept in registers for the whole launch (30 of the 60 VGPRs
    // this kernel left unused at 2 waves per SIMD) instead of eight ds_read_b128 per transform: LDS array time is
    // not hidden behind the butterflies in this kernel, so the 11 % of it that these reads
    // were came off the launch time one for one (1.778 -> 1.728 ms)
    C16 tw2r;
    {
        const float2* rowf2 = reinterpret_cast<const float2*>(tw2row);
        tw2r.set(0, 1.0f, 0.0f);
#pragma unroll
        for (int q = 1; q < 16; ++q) {
            const float2 w = rowf2[4 * (q & 3) + (q >> 2) - 1];
            tw2r.set(q, w.x, w.y);
        }
    }

    // persistent workgroup: the tables above are loaded once, then windows blockIdx.x, +gridDim.x, ...
    for (int wl = blockIdx.x; wl < n_win; wl += gridDim.x) {
    C16 sa, sb;   // anchor spectrum X_i and the streamed X_j (scalar arrays: see C16)
    // spectrum scratch is per WORKGROUP, not per window: the persistent workgroup reuses the same
    // B x 64 KiB for every window it processes (B = 8: slots 1 .. 6 are written, 256 x 384 KiB = 98 MB live for the
    // whole launch, resident in the 256 MB Infinity Cache, rewritten before most of it is ever evicted to HBM)
    const long wbase = (long)blockIdx.x * B;
    const long obase = (first_window + wl) * (long)n_pairs;
    int seq = 0;         // transform counter: selects the exchange image
    int npair = 0;       // pair counter: selects the record slot (ring of kResSlots)
    int npend = 0;       // pairs whose records await a resolve

    auto barrier_hook = [&](bool flush) __attribute__((always_inline)) {
        if constexpr (FX & 4) __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the asm stores are not counted by the compiler
        __syncthreads();
        if (npend == kResBatch || (flush && npend > 0)) {
            if (wave == (seq & kResWaveMask)) {
                if constexpr (BOUNDED)
                    resolve_batch<true>(lane, red, halo, oidx, (npair - npend) & (kResSlots - 1), npend, obase, out_scale,
                                        lag_int, lag_frac, peak, lb, first_window + wl);
                else
                    resolve_batch(lane, red, halo, oidx, (npair - npend) & (kResSlots - 1), npend, obase, out_scale, lag_int,
                                  lag_frac, peak);
            }
            npend = 0;
        }
    };
    // odd lanes: v[q] *= W32^q, the per-slot part of the odd sub-transform's W_L^n (in place)
    auto mul_w32_odd = [&](float2 (&v)[16]) __attribute__((always_inline)) {
        if (p) {
            {   // q = 1..3 one by one, then three groups of four in one asm statement each
#pragma unroll
                for (int q = 1; q < 4; ++q) {
                    const float2 w = w32(q);
                    float x = v[q].x, y = v[q].y;   // scalars by value: keeps the array out of scratch
                    cmul_inplace(x, y, w.x, w.y);
                    v[q].x = x;
                    v[q].y = y;
                }
            }
#pragma unroll
            for (int q = 4; q < 16; q += 4) {
                float x0 = v[q].x, y0 = v[q].y, x1 = v[q + 1].x, y1 = v[q + 1].y;
                float x2 = v[q + 2].x, y2 = v[q + 2].y, x3 = v[q + 3].x, y3 = v[q + 3].y;
                cmul4_inplace(x0, y0, x1, y1, x2, y2, x3, y3, w32(q), w32(q + 1), w32(q + 2), w32(q + 3));
                v[q].x = x0; v[q].y = y0; v[q + 1].x = x1; v[q + 1].y = y1;
                v[q + 2].x = x2; v[q + 2].y = y2; v[q + 3].x = x3; v[q + 3].y = y3;
            }
        }
    };
    // All global traffic of the loop goes through buffer descriptors held in SGPRs: address = SRD
    // base + one shared 32-bit VGPR offset + an SGPR/immediate offset.  (With flat 64-bit addressing
    // hipcc keeps ~100 VGPRs of loop-invariant addresses alive and spills the twiddles instead.)
    const int samp_bytes = U8 ? 2 : 8;
    const __amdgpu_buffer_rsrc_t xs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(iq_v)) + (first_window + wl) * (long)B * kM * samp_bytes, 0,
        B * kM * samp_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ss = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<char*>(spec) + wbase * (long)(8 * kThreads * 16), 0, B * (8 * kThreads * 16), 0x00020000);
    const int xoff = u * samp_bytes, soff = t * 16;
    // raw window samples of buoy b into d (uint8 pairs stay packed in d[q].x until cvt_x)
    auto load_x = [&](C16& d, int b) __attribute__((always_inline)) {
        if constexpr (U8) {
#pragma unroll
            for (int q = 0; q < 16; ++q)
                d.re[q] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(xs, xoff, (b * kM + q * 256) * 2, 0));
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const u32x2 r = __builtin_amdgcn_raw_buffer_load_b64(xs, xoff, (b * kM + q * 256) * 8, 0);
                d.set(q, __uint_as_float(r.x), __uint_as_float(r.y));   // (by value: see NOTE)
            }
        }
    };
    // quarter G of the same loads (slots 4G..4G+3): issued between the groups of a butterfly layer
    auto load_x_part_from = [&](const __amdgpu_buffer_rsrc_t& rs, C16& d, int b, auto part) __attribute__((always_inline)) {
        constexpr int G = decltype(part)::value;
        constexpr int Q0 = 2 * G, Q1 = 2 * G + 2;   // eighths: issued from the groups of BOTH butterfly layers of h1
        // (the buoy's byte offset is made opaque HERE so that each request's SGPR offset is computed in front of it (s_mov +
        // s_addk): left to itself hipcc precomputes all of them ahead of the loop, runs out of SGPRs, and every request
        // then pays v_readlane + s_nop 4 to get its offset back out of a spill lane.  One `s_add_i32` per request in a
        // volatile asm is one instruction fewer and measured +1.5 %: volatile statements keep their order among
        // themselves, which pins every request between the exchange stores around it.)
        int bo = b * (kM * samp_bytes);
        asm volatile("" : "+s"(bo));
        if constexpr (U8) {
#pragma unroll
            for (int q = Q0; q < Q1; ++q)
                d.re[q] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rs, xoff, bo + q * 256 * 2, 0));
        } else {
#pragma unroll
            for (int q = Q0; q < Q1; ++q) {
                const u32x2 r = __builtin_amdgcn_raw_buffer_load_b64(rs, xoff, bo + q * 256 * 8, 0);
                d.set(q, __uint_as_float(r.x), __uint_as_float(r.y));
            }
        }
    };
    auto load_x_part = [&](C16& d, int b, auto part) __attribute__((always_inline)) { load_x_part_from(xs, d, b, part); };
    auto cvt_x = [&](C16& d) __attribute__((always_inline)) {
        if constexpr (U8) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const unsigned r = __float_as_uint(d.re[q]);
                d.set(q, (float)(r & 0xffu) - 127.5f, (float)(r >> 8) - 127.5f);
            }
        }
    };
    auto load_spec_part = [&](C16& d, int b, auto part) __attribute__((always_inline)) {
        constexpr int G = decltype(part)::value;
        constexpr int J0 = G, J1 = G + 1;
        int bo = b * (8 * kThreads * 16);   // (opaque: see load_x_part_from)
        // (last argument of the scratch loads / stores: cache policy aux bits, 1 = sc0, 2 = sc1, 4 = nt; 0 measured best, LABNOTES R4.7)
        asm volatile("" : "+s"(bo));
#pragma unroll
        for (int j = J0; j < J1; ++j) {
            const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(ss, soff, bo + j * (kThreads * 16), 0);
            d.set(2 * j, __uint_as_float(w.x), __uint_as_float(w.y));
            d.set(2 * j + 1, __uint_as_float(w.z), __uint_as_float(w.w));
        }
    };
    auto store_spec = [&](const C16& d, int b) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            // (opaque copies: hipcc otherwise widens these four scalar reads into overlapping 16-byte
            // loads of the register array, which pins half of it in scratch memory)
            float e0 = d.re[2 * j], e1 = d.im[2 * j], e2 = d.re[2 * j + 1], e3 = d.im[2 * j + 1];
            asm volatile("" : "+v"(e0), "+v"(e1), "+v"(e2), "+v"(e3));
            const u32x4 w = {__float_as_uint(e0), __float_as_uint(e1), __float_as_uint(e2), __float_as_uint(e3)};
            // The whole byte offset goes into the VGPR offset, soffset = 0.  Root cause of the corruption seen with
            // an SGPR soffset (round 2, tools/exp_soffset.py + tools/probe/soffset_probe.hip): a store of more
            // than 64 bits reads its data VGPRs late, so a VALU write to them needs a wait state behind the store
            // (ISA "required software-inserted wait states").  hipcc 7.2's hazard recognizer waives that wait
            // state when the store has an SGPR soffset, but on gfx950 the hazard is still there: with soffset in
            // an SGPR the next group's `v_mov_b32 v3, v86` followed the store of v[2:5] directly and half of all
            // pair-windows came out wrong on every call; the same stores with two wait states forced behind each
            // (an asm that keeps e0..e3 live) were right 200 calls out of 200, as is this immediate-soffset form, for
            // which the compiler inserts the s_nop itself.  (The SGPR form alone is fine: the probe, whose stores
            // do not reuse their data registers, has no wrong float.)
            __builtin_amdgcn_raw_buffer_store_b128(w, ss, soff + (b * 8 + j) * (kThreads * 16), 0, 0);
        }
    };
    // forward spectrum of the samples in x, in place (carries the 2^-6 of the TW1 table)
    auto fwd = [&](C16& xc) __attribute__((always_inline)) {
        float2* img = (seq & 1) ? img1 : img0;
        float2 x[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) x[q] = xc.get(q);
        mul_w32_odd(x);            // odd sub-transform input x*W32^q (W_L^u is folded into tw1)
        dft16(x);
        mul_tw1(x, tw1);
        if constexpr (FX & 2) {
            int tf = t;   // FX & 16: the base is computed here, at every transform, not held in a register across the launch
            if constexpr (FX & (16 | 32)) asm volatile("" : "+v"(tf));
            // FX & 32: the same index from the inverse's base, which is live anyway: bits 3 and 4 of the index change places
            float2* b = img + ((FX & 32) ? xa2_base(t) + 8 * (((tf >> 4) & 1) - (tf & 1)) : xa2f_base(tf));
#pragma unroll
            for (int k0 = 0; k0 < 16; ++k0) b[k0 * kBcHalf] = make_float2(x[k0].x, x[k0].y);
        } else {
            xchg_a2_write(img, x, t);
        }
        barrier_hook(false);
        int tg = t;
        if constexpr (FX & (16 | 32)) asm volatile("" : "+v"(tg));
        const int xbf = (FX & 32) ? xb2_base(t) + 8 * (((tg >> 3) & 1) - ((tg >> 4) & 1)) : xb2f_base(tg);
        if constexpr (FX & 1) {
            xchg_b2_read_plain((seq & 1) * kLdsWinImg + 8 * ((FX & 2) ? xbf : xb2_base(t)), x);
            if constexpr (FX & 8) {   // opaque scalars: the pairs the reads land in otherwise draw v_pk_add_f32 into layer 1
#pragma unroll
                for (int q = 0; q < 16; ++q) asm volatile("" : "+v"(x[q].x), "+v"(x[q].y));
            }
        } else if constexpr (FX & 2) {
            const float2* b = img + xbf;
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) x[n1] = b[n1 * 32];
        } else {
            xchg_b2_read(img, x, t);
        }
        dft16(x);
        loc_write16(loc_m0[seq & 1], x);
        wave_lds_order();
        loc_read16(smem + (seq & 1) * kLdsWinImg + loc_rd, x);
        dft16_tw<true>(x, tw2r);
#pragma unroll
        for (int q = 0; q < 16; ++q) xc.set(q, x[q].x, x[q].y);   // (scaled by 2^-6 through the TW1 table)
        ++seq;
    };
    // One pair = two halves around its only workgroup barrier.
    //   h1  conj-multiply merged into the role-C pass, wave-local exchange, role-B pass, stores into
    //       exchange image `tr & 1` (this wave's own regions); `prefetch(part)` is called eight times,
    //       from the groups of both butterfly layers (parts 0-3 behind the role-C pass, 4-7 behind the role-B pass: one
    //       16-byte request per part instead of bursts of two, tools/probe/kwin_bench.hip: -0.6 %), always
    //       after the last read of a and s (their registers may be reloaded there)
    //   h2  reads image `tr & 1` (all waves' regions), role-A pass, last radix-2, |.|^2, peak records
    // h2 of pair n and h1 of pair n+1 sit between the same two barriers and do not depend on each
    // other (different images, disjoint registers), so the two waves that share a SIMD can run them in
    // opposite order: see the phase-2 loop.
    auto pair_h1 = [&](const C16& a, const C16& s, int tr, auto prefetch) __attribute__((always_inline)) {
        float2* img = (tr & 1) ? img1 : img0;
        float2 v[16];
        // R = X_j conj(X_i), (im,re)-swapped == swap(X_j) * X_i: merged into the first radix-16 pass
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = make_float2(s.im[q], s.re[q]);
        dft16_tw_l1<false>(v, a);                // k2 -> n0   (role C), layer 1: the last reads of a and s
#pragma unroll
        for (int q = 0; q < 16; q += 4)          // pin: the requests below must follow the reads above
            asm volatile("" : "+v"(v[q].x), "+v"(v[q].y), "+v"(v[q + 1].x), "+v"(v[q + 1].y), "+v"(v[q + 2].x),
                         "+v"(v[q + 2].y), "+v"(v[q + 3].x), "+v"(v[q + 3].y));
        __builtin_amdgcn_sched_barrier(0);
        {   // layer 2 group by group: each group's outputs go to the wave-local image at once, and a
            // quarter of the next spectra is requested behind it
            dft16_layer2_emit(v, [&](auto kac, const float2& x0, const float2& x1, const float2& x2, const float2& x3)
                                     __attribute__((always_inline)) {
                constexpr int ka = decltype(kac)::value;
                loc_write4<ka, ka + 4, ka + 8, ka + 12>(loc_m0[tr & 1], x0, x1, x2, x3);
                prefetch(kac);
            });
        }
        wave_lds_order();
        loc_read16(smem + (tr & 1) * kLdsWinImg + loc_rd, v);
        dft16_tw_l1<true>(v, tw2r);
        {
            float2* xb = img + xb2_base(t);                             // own k0 row of the [k0][n1][p][n0] image
            dft16_layer2_emit(v, [&](auto kac, const float2& x0, const float2& x1, const float2& x2, const float2& x3)
                                     __attribute__((always_inline)) {
                constexpr int ka = decltype(kac)::value;
                if constexpr (FX & 4) {
                    xchg_b2_write4_plain<ka>((tr & 1) * kLdsWinImg + 8 * xb2_base(t), x0, x1, x2, x3);
                } else {
                    xb[ka * 32] = make_float2(x0.x, x0.y);
                    xb[(ka + 4) * 32] = make_float2(x1.x, x1.y);
                    xb[(ka + 8) * 32] = make_float2(x2.x, x2.y);
                    xb[(ka + 12) * 32] = make_float2(x3.x, x3.y);
                }
                prefetch(std::integral_constant<int, ka + 4>{});
            });
        }
    };
    auto pair_h2 = [&](int tr, int out_idx) __attribute__((always_inline)) {
        const float2* img = (tr & 1) ? img1 : img0;
        const int rb = npair & (kResSlots - 1);
        float2 v[16];
        xchg_a2_read(img, v, t);
        dft16_tw<false>(v, tw1);                 // W_M^(u*k0) [* W_L^u odd], k0 -> n2   (role A)
        mul_w32_odd(v);                          // odd lanes: * W32^q
        // last radix-2 stage across the lane pair, up to a sign that |.| does not see:
        // even lane e + o' = r[n], odd lane o' - e = -r[n+M]
        pair_fmac8(v[0].x, v[0].y, v[1].x, v[1].y, v[2].x, v[2].y, v[3].x, v[3].y, sgn);
        pair_fmac8(v[4].x, v[4].y, v[5].x, v[5].y, v[6].x, v[6].y, v[7].x, v[7].y, sgn);
        pair_fmac8(v[8].x, v[8].y, v[9].x, v[9].y, v[10].x, v[10].y, v[11].x, v[11].y, sgn);
        pair_fmac8(v[12].x, v[12].y, v[13].x, v[13].y, v[14].x, v[14].y, v[15].x, v[15].y, sgn);
        float mag[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) mag[q] = fmaf(v[q].x, v[q].x, v[q].y * v[q].y);
        if (p && u == 0) mag[0] = -1.0f;         // lag -M is not part of the 'full' output
        if constexpr (BOUNDED) {                 // lag window: |r|^2 outside it -> the same sentinel (lag_bounds.hpp)
            int klo, khi;
            lag_window(lb, first_window + wl, out_idx, kM - 1, klo, khi);
#pragma unroll
            for (int q = 0; q < 16; ++q) mag[q] = lag_mask(mag[q], kbase + q * 256, klo, khi);
        }
        if (is_halo) {
            float4* hp = reinterpret_cast<float4*>(halo + ((rb * 8 + wave) * kHaloRows + hl) * 16);
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4)
                hp[q4] = make_float4(mag[4 * q4], mag[4 * q4 + 1], mag[4 * q4 + 2], mag[4 * q4 + 3]);
        }
        float tmax = mag[0];
#pragma unroll
        for (int q = 1; q < 16; ++q) tmax = fmaxf(tmax, mag[q]);
        // Lowest slot holding the lane's max (four select chains, descending so that lower slots win), with the four
        // row steps of the wave maximum issued BETWEEN the chains' groups: the DPP steps depend on each other, the
        // groups do not depend on them, so neither the 2 wait states in front of a DPP read nor the steps' latency
        // are ever waited for.  One asm statement (hipcc separates consecutive statements by s_nop).
        int qa = 16, qb = 16, qc = 16, qd = 16;
        float wrow;
        {
            unsigned long long k0, k1, k2, k3;
#define RMX_AS4(M0, M1, M2, M3, Q)                                                        \
    "v_cmp_eq_f32_e64 %[k0], %[" #M0 "], %[t]\n\tv_cmp_eq_f32_e64 %[k1], %[" #M1 "], %[t]\n\t" \
    "v_cmp_eq_f32_e64 %[k2], %[" #M2 "], %[t]\n\tv_cmp_eq_f32_e64 %[k3], %[" #M3 "], %[t]\n\t" \
    "v_cndmask_b32_e64 %[qa], %[qa], " #Q ", %[k0]\n\tv_cndmask_b32_e64 %[qb], %[qb], " #Q "+1, %[k1]\n\t" \
    "v_cndmask_b32_e64 %[qc], %[qc], " #Q "+2, %[k2]\n\tv_cndmask_b32_e64 %[qd], %[qd], " #Q "+3, %[k3]\n\t"
            asm volatile(RMX_AS4(mc, md, me, mf, 12)
                         "v_max_f32_dpp %[w], %[t], %[t] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                         RMX_AS4(m8, m9, ma, mb, 8)
                         "v_max_f32_dpp %[w], %[w], %[w] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                         RMX_AS4(m4, m5, m6, m7, 4)
                         "v_max_f32_dpp %[w], %[w], %[w] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
                         RMX_AS4(m0, m1, m2, m3, 0)
                         "v_max_f32_dpp %[w], %[w], %[w] row_mirror row_mask:0xf bank_mask:0xf"
                         : [qa] "+v"(qa), [qb] "+v"(qb), [qc] "+v"(qc), [qd] "+v"(qd), [w] "=&v"(wrow), [k0] "=&s"(k0),
                           [k1] "=&s"(k1), [k2] "=&s"(k2), [k3] "=&s"(k3)
                         : [t] "v"(tmax), [m0] "v"(mag[0]), [m1] "v"(mag[1]), [m2] "v"(mag[2]), [m3] "v"(mag[3]),
                           [m4] "v"(mag[4]), [m5] "v"(mag[5]), [m6] "v"(mag[6]), [m7] "v"(mag[7]), [m8] "v"(mag[8]),
                           [m9] "v"(mag[9]), [ma] "v"(mag[10]), [mb] "v"(mag[11]), [mc] "v"(mag[12]), [md] "v"(mag[13]),
                           [me] "v"(mag[14]), [mf] "v"(mag[15]));
#undef RMX_AS4
        }
        const int qsel = min(min(qa, qb), min(qc, qd));
        const int kq = kbase + qsel * 256;
        const int wi = __builtin_bit_cast(int, wrow);   // every lane: the max of its row of 16
        const float wmax = fmaxf(fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(wi, 0)),
                                       __builtin_bit_cast(float, __builtin_amdgcn_readlane(wi, 16))),
                                 fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(wi, 32)),
                                       __builtin_bit_cast(float, __builtin_amdgcn_readlane(wi, 48))));
        // which lane holds it?  One lane almost always: its index and slot come over by readlane.  Several lanes (an
        // exact tie between lanes): the lowest 'full' index decides, found by the wave minimum as before.
        const unsigned long long hit = __ballot(tmax == wmax);
        int kw, ls, qs;
        if (__popcll(hit) == 1) {
            ls = __ffsll((long long)hit) - 1;
            kw = __builtin_amdgcn_readlane(kq, ls);
            qs = __builtin_amdgcn_readlane(qsel, ls);
        } else {
            kw = wave_min_i32(tmax == wmax ? kq : 0x7fffffff);
            int ts;
            k_to_owner(kw, ts, qs);
            ls = ts & 63;
        }
        // qs is wave-uniform (it comes out of the wave reductions): one indexed register read
        // (s_set_gpr_idx) instead of a 16-way select chain
        typedef float f16v __attribute__((ext_vector_type(16)));
        const f16v mv = {mag[0], mag[1], mag[2],  mag[3],  mag[4],  mag[5],  mag[6],  mag[7],
                         mag[8], mag[9], mag[10], mag[11], mag[12], mag[13], mag[14], mag[15]};
        const float sel = mv[__builtin_amdgcn_readfirstlane(qs)];
        const int seli = __builtin_bit_cast(int, sel);
        const float tapm = ls >= 2 ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(seli, ls >= 2 ? ls - 2 : 0)) : -2.0f;
        const float tapp = ls <= 61 ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(seli, ls <= 61 ? ls + 2 : 63)) : -2.0f;
        if (lane == 0) {
            const u32x4 rec = {__float_as_uint(wmax), (unsigned)kw, __float_as_uint(tapm), __float_as_uint(tapp)};
            *reinterpret_cast<u32x4*>(red + rb * 8 + wave) = rec;
            if (wave == 0) oidx[rb] = out_idx;
        }
        ++npend;
        ++npair;
    };
    auto pair = [&](const C16& a, const C16& s, int out_idx, auto prefetch) __attribute__((always_inline)) {
        pair_h1(a, s, seq, prefetch);
        barrier_hook(false);                     // the pair's only barrier
        pair_h2(seq, out_idx);
        ++seq;
    };
    auto out_of = [&](int i, int j) -> int { return i * B - (i * (i + 1)) / 2 + (j - i - 1); };

    // ---- anchor 0: X_0 goes straight into the anchor registers (never stored); every other X_e but the last is
    // transformed once, stored once for the later anchors, and used at once from registers for (0,e)
    load_x(sa, 0);
    if (B > 1) load_x(sb, 1);          // sb is free: X_1's samples travel while X_0 is transformed
    cvt_x(sa);
    fwd(sa);
    // (the last buoy is peeled off the loop: its pair requests spectra instead of samples; with both
    // request kinds in one loop body the compiler's waitcnt bookkeeping merges their destination
    // registers across the back edge)
    for (int e = 1; e + 1 < B; ++e) {
        cvt_x(sb);
        fwd(sb);
        store_spec(sb, e);
        pair(sa, sb, out_of(0, e), [&](auto part) __attribute__((always_inline)) { load_x_part(sb, e + 1, part); });
    }
    // ---- the last buoy and the pairs among buoys 1..B-1, in the order of a host-planned table (host::plan_pair_trail:
    // runs that hand the anchor over).  Entry 0 of the table is the pair (0, B-1), entry k + 1 the order's step k:
    // {out_idx, load_arr, load_idx, 0}.  Consecutive steps share one buoy, whose spectrum stays in its register array; each
    // step's h1 requests ONE spectrum (load_idx) into the array whose buoy the next step drops (load_arr: 0 = sa, 1 = sb).
    // In this order X_i is in sa and X_j in sb at every step (host::trail_kernel_ok, checked where the table is built), so
    // pair_h1 gets them as the anchor runs gave them and every pair's arithmetic is what it was.  X_{B-1} stays in sb
    // behind phase 1 and is never stored: the first step is (first_load, B-1), and only first_load is requested, into sa.
    {
        const int M2 = (B - 1) * (B - 2) / 2;            // steps of the order
        const int4* __restrict__ tab = trail;
        int4 cur = tab[0];
        int4 nxt = tab[M2 > 0 ? 1 : 0];
        if (B > 1) {
            cvt_x(sb);
            fwd(sb);
            // (X_{B-1} is NOT stored: no entry of the table requests it -- host::trail_kernel_ok -- and the scratch is private
            // to this workgroup, so nobody else could read it either.  Its slot of the scratch stays allocated and unwritten.)
            const int fl = cur.z;
            pair(sa, sb, cur.x, [&](auto part) __attribute__((always_inline)) {
                if (M2 > 0) load_spec_part(sa, fl, part);
            });
        }
        // h1 of the step in `st`, its request into sa or into sb.  Two ONE-SIDED branches, not an if / else: with an else
        // side the compiler lays the sides out one behind the other and keeps the spectrum a side requested in registers of
        // its own across the other side, then moves the registers behind a wait for every request, at every step.  (An
        // opaque copy of the selector per test: left to itself the compiler folds the tests back into one two-sided branch.)
        auto h1_step = [&](const int4& st, int tr) __attribute__((always_inline)) {
            const int li = st.z;
            const int var = __builtin_amdgcn_readfirstlane(st.y);
            int v0 = var, v1 = var;
            asm volatile("" : "+s"(v0));
            if (v0 == 0) pair_h1(sa, sb, tr, [&](auto part) __attribute__((always_inline)) { load_spec_part(sa, li, part); });
            asm volatile("" : "+s"(v1));
            if (v1 != 0) pair_h1(sa, sb, tr, [&](auto part) __attribute__((always_inline)) { load_spec_part(sb, li, part); });
        };
        // Step m's h1 sits between the same two barriers as h2 of the pair before it (m = 0: behind h2 of (0, B-1), above).
        // The two are independent (different images, disjoint registers): waves 0-3 of stag 1 run h2 first, the others h1
        // first, so that one wave's LDS / barrier / DPP-chain stalls fall on the other's butterfly arithmetic instead of on
        // the same stalls (all eight waves are otherwise barrier-aligned in lockstep).  ONE copy of h1 between two one-sided
        // copies of h2, not two sides of h1 + h2 each.
        // SIMD pairs {a, a+2} vs {a+1, a+3} (stag 1): measured best of the splits; 0 = nobody, 5 = everybody late
        // (2: odd waves = SIMDs 1, 3; 3: the second wave of every SIMD; 4: one wave of every SIMD, alternating between SIMDs)
        const bool late_h2 = stag == 1 ? ((wave >> 1) & 1) : stag == 2 ? (wave & 1) : stag == 3 ? (wave >> 2) :
                             stag == 4 ? ((wave ^ (wave >> 2)) & 1) : (stag == 5);
#pragma clang loop unroll(disable)
        for (int m = 0; m <= M2; ++m) {
            const int4 ahead = tab[m + 2 <= M2 ? m + 2 : M2];   // one step ahead of its use
            if (m > 0) {
                barrier_hook(false);
                // The two waves of a SIMD share its issue slots (and the CU's LDS / vector-memory request paths), and every
                // arbiter prefers the OLDER one: in-kernel shader-clock stamps (LABNOTES 6.2) showed waves 0-3
                // spending 51-60 k ticks per window in the two pieces between barriers where waves 4-7 need 57-64 k, and then
                // waiting ~950 ticks at every barrier for them (waves 4-7: ~270).  Priority outranks age, so waves 4-7 run the
                // FIRST of their two pieces at priority 1 and the second at 0 (h2 is the piece that reacts to priority).
                if (wave >= 4) __builtin_amdgcn_s_setprio(1);
                if (!late_h2) {
                    pair_h2(seq, cur.x);
                    if (wave >= 4) __builtin_amdgcn_s_setprio(0);
                }
            }
            if (m < M2) h1_step(nxt, m > 0 ? seq + 1 : seq);
            if (m > 0) {
                if (late_h2) {
                    if (wave >= 4) __builtin_amdgcn_s_setprio(0);
                    pair_h2(seq, cur.x);
                }
                ++seq;
            }
            cur = nxt;
            nxt = ahead;
        }
    }
    seq = 0;   // any wave may resolve the last pairs; take wave 0
    barrier_hook(true);
    }   // next window of this workgroup
