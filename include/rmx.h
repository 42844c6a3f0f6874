/* rmx.h -- C ABI of the MI355X (gfx950) TDoA cross-correlation engine.
 *
 * What this boundary replaces in the reference (physiii/radio-mapper):
 *   The reference has no FFI for this path: the path sits behind plain
 *   Python methods of tdoa_processor.py.  The seam is the body of the pair loop of
 *   TDoACalculator.calculate_tdoa_measurements (tdoa_processor.py:156-193), whose time difference
 *   `time_diff_ns = det2.gps_timestamp_ns - det1.gps_timestamp_ns` (tdoa_processor.py:166) is
 *   replaced by a lag measured from IQ with the cross-correlation primitive the module imports
 *   (`from scipy.signal import correlate`, tdoa_processor.py:20).  rmx_xcorr_batch() is that
 *   primitive, batched over capture windows x buoy pairs:
 *
 *     for every window w, for every pair (i, j), i < j, in the reference's nested-loop order
 *     (tdoa_processor.py:156-157):
 *         c   = correlate(x[w][j], x[w][i], mode='full', method='fft')   (complex64, 2N-1 lags)
 *         m   = |c|                                                     (float32)
 *         k   = argmax m   (ties -> lowest k)        lag_int  = k - (N-1)
 *               (Parity statement: lag_int is BIT-EXACT against scipy's float32 path wherever that path's own two
 *               largest magnitudes differ by more than 1e-5 relative -- every committed fixture, every BASELINE shape --
 *               and the lowest index on exact ties.  Where two candidates are closer than that, two correct float32
 *               FFTs may order them differently; the tests accept only the oracle's own second candidate there.)
 *               (The kernels search the maximum of |c|^2 and take the square root of the three taps only.  sqrt is
 *               monotonic, so the two orders agree except in one class of inputs: two lags whose |c|^2 differ in the
 *               last bit but whose float32 |c| round to the SAME value.  numpy then sees a tie and takes the lower
 *               index; the kernels take the lag with the larger square.  Such pairs are one float32 ulp apart in
 *               magnitude -- below what two float32 FFTs agree on -- and cannot occur when the two values are
 *               bit-identical, which is the case the tie rule is tested on.)
 *         d   = 3-point parabolic vertex offset      lag_frac = d  (0 at the edges / flat top)
 *               (d = (a - c) / (2 (a - 2b + c)) in double precision from the float32 taps a, b, c = m[k-1], m[k], m[k+1].
 *               Against another float32 implementation of the same definition it agrees to 1e-5 * max(|lag|, 1)
 *               wherever that formula is well conditioned -- 8.7 M random pair-windows, N = 16 ... 2^18, worst 7e-6 --
 *               and to the formula's own conditioning where it is not: two pair-windows of those, e.g. a flat peak on a
 *               32-sample window at 0 dB (a - 2b + c = 4e-3 b), where one float32 ulp on each tap moves d by 2.3e-5,
 *               differed by 3.3e-5.  The rule -- within 1e-5, or within four such
 *               one-ulp bounds, nothing else -- is pinned in tests/test_gpu_parity.py::test_flat_peak_rule_on_short_noisy_windows
 *               and used by tests/soak_parity.py.)
 *               (Far from lag 0 that scaled bar says little -- 0.16 samples at lag 16000 --, so
 *               tests/test_gpu_far_lags.py holds d ITSELF to 1e-5 absolute, or the flat-peak bound, against a float64
 *               reference with the peak placed anywhere in +-(N-1), seams of every kernel's output order included, on
 *               every route: worst 4.0e-7 on an MI355X, where scipy's float32 path holds 3.0e-7.  With full 24-bit
 *               mantissas in every sample -- floats normalised to +-1 by a non-power-of-two factor, int16-scaled
 *               floats -- instead of the 8 bits of the uint8 grid, tests/test_gpu_dynamic_range.py holds every route to
 *               the same bars: worst 3.8e-7 on lag_frac and 4.8e-7 relative on peak on an MI355X.)
 *         peak = m[k]
 *     lag = lag_int + lag_frac samples = delay(buoy j) - delay(buoy i)   (sign of
 *     TDoAMeasurement.time_difference_ns: buoy2 - buoy1, tdoa_processor.py:51).
 *
 *   The ctypes binding a maintainer adds on the reference side is shown in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes, no torch / numpy types.  The caller owns every buffer it
 * passes; the library owns only ctx-internal device scratch.  Functions return 0 (RMX_OK) or a
 * negative code and never abort; rmx_last_error() gives the text.  A ctx is single-owner (not
 * thread safe); use one ctx per device (one process per GPU, or one host thread per ctx).
 *
 * The caller's buffers (tests/test_gpu_caller_memory.py holds every correlation and Doppler-search route to this):
 *   Alignment: a DEVICE pointer must be aligned to its element and to nothing more -- `iq` to 8 bytes (one complex64
 *     sample) or, with RMX_IN_U8, to 2 bytes (one I,Q pair; an odd address is refused), every output to 4 bytes.  The
 *     kernels touch caller memory one element per access, so a slice of a larger buffer is as good as a fresh allocation.
 *     A device pointer aligned to less is RMX_E_INVAL, the text naming the array, checked directly behind the NULL-buffer
 *     check.  Host pointers only pass through the library's own copies and need no alignment beyond their C type's.
 *   Extent: a call writes exactly [rows][n_pairs] elements of lag_int, lag_frac and peak ([n_windows][n_bands][n_pairs] in a
 *     banded call; x 4 for quality; dop_idx and dop_frac like lag_int) and not one byte in front of or behind them, and it
 *     never writes its input.  A refused call writes nothing.
 *   Order: everything a call queues -- copies, kernels, the staging of pairs, bands and bounds -- is ordered on the ctx
 *     stream, whichever stream rmx_set_stream named, one that does not synchronise with the null stream included: work
 *     queued on that stream before the call is seen by it, work queued behind it sees its outputs.  Two asynchronous
 *     (RMX_OUT_DEVICE) calls on one ctx may follow each other without a wait, with different pair lists, bands and bounds.
 */
#ifndef RMX_H
#define RMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rmx_ctx rmx_ctx;

enum {
    RMX_OK = 0,
    RMX_E_INVAL = -1,       /* bad argument */
    RMX_E_NODEV = -2,       /* no usable HIP device */
    RMX_E_HIP = -3,         /* a HIP runtime call failed (text in rmx_last_error) */
    RMX_E_NOMEM = -4,       /* device or host allocation failed */
    RMX_E_UNSUPPORTED = -5  /* shape not supported by this build */
};

/* flags of rmx_xcorr_batch() */
enum {
    RMX_IN_DEVICE = 1u,   /* `iq` is a device pointer (already resident in HBM) */
    RMX_OUT_DEVICE = 2u,  /* lag_int / lag_frac / peak are device pointers; the call is then
                             asynchronous on the ctx stream (rmx_synchronize to wait) */
    RMX_IN_U8 = 4u        /* `iq` is raw rtl_sdr uint8 I,Q interleaved [W][B][N][2]; decoded in
                             the first kernel as (float)u8 - 127.5f (buoy_node.py:392-398) */
};

#define RMX_VERSION 1

int rmx_version(void);

/* Number of HIP devices visible, 0 if none / no driver.  Never fails. */
int rmx_device_count(void);

/* Create an engine for windows of `n_samples` complex64 samples from `n_buoys` buoys.
 * n_samples: power of two, 16 .. 4194304.  max_windows: largest n_windows a later call may pass.
 * n_windows of every batch entry below is bounded by max_windows and by the device's memory alone: the library cuts a
 * batch into chunks of its own (the four-step route so that its column pass has at most 65535 grid rows, one per
 * (window, pair) slot), and every offset into the caller's arrays and into its scratch is 64-bit.  Inputs beyond 4 GiB
 * (host and device pointers, complex64 and uint8 -- sample index 2^31 --), scratch beyond 4 GiB inside one chunk and calls
 * of more than 65535 (window, pair) slots are tested on every route (tests/test_gpu_large_batches.py).
 * flags: reserved, pass 0. */
int rmx_create(rmx_ctx** out, int device_id, int n_buoys, int n_samples, int max_windows,
               unsigned flags);
void rmx_destroy(rmx_ctx* ctx);

/* Text of the last error on this ctx (or of the last failed rmx_create when ctx == NULL). */
const char* rmx_last_error(const rmx_ctx* ctx);

/* Use an existing hipStream_t (e.g. torch's current stream) for all work of this ctx. */
int rmx_set_stream(rmx_ctx* ctx, void* hip_stream);

/* Per-ctx options (all optional): "chunk_windows" (windows per launch), "timing" (1: bracket every
 * launch with HIP events, read back with rmx_last_timing), "fused" (default 1; 0 forces the separate
 * forward + pair kernels that custom pair lists use), "resident" and "pairs_per_block" (variants of
 * that unfused pair kernel; without an explicit "pairs_per_block" the library sizes the blocks to the batch),
 * "small4096" (default 1: batches of N = 4096 too small to fill the chip with one workgroup per window -- fewer than
 * about 0.25 ... 0.5 windows per CU, depending on the buoy count -- run through those per-transform kernels, which spread
 * one window's spectra and pairs over the CUs: 13 us instead of 92 us for a single window of 8 buoys; 0: always the
 * fused kernel), "stag" (0..5: which waves of the fused N = 4096 kernel run the two halves
 * between barriers in the opposite order; default 0, nobody: scheduling only, every value gives the same bytes), "win8" / "pk" (two other builds of that kernel,
 * tools/experiments/: present only in a -DRMX_EXPERIMENTS build, RMX_E_UNSUPPORTED otherwise), "dbg"
 * (the ablation masks of a timing-only build that was removed; the key is rejected with RMX_E_UNSUPPORTED).
 * Returns RMX_E_INVAL for an unknown key. */
int rmx_set_option(rmx_ctx* ctx, const char* key, long value);

/* Kernel-selection defaults for engines created AFTERWARDS (process-wide; an existing ctx keeps the values it was
 * created with, so its kernels, block sizes and LDS sizes stay consistent).  For tests and A/B measurements: the
 * library never reads the environment.  Keys (radio-mapper_amd/csrc/host_plan.hpp lists ranges and meanings):
 * "stag", "ncus", "chunk_windows", "small4096", "generic4096", "small_maxl", "logl1", "wfused", "wscr", "wscr14",
 * "wscr_per_cu", "rows_anchor", "fused", "fused_def", "gen_chunk", "rows_tpr", "cols_threads", "col_logt", "kwin8k"
 * (N = 8192, batches that fill the chip: 1 = k_win8kl, the default; 0 = g_win_scr14), "kwin16k" (N = 16384: 1 = k16_fwd +
 * k16_pairs from "k16_min_windows" windows on -- default 100 / (buoys + pairs) -- unless "wscr" = 2; 2 = for every batch;
 * 0 = g_win_eo15 / the four-step kernels).
 * Returns RMX_E_INVAL (text through rmx_last_error(NULL)) for an unknown key or a value out of range;
 * value == LONG_MIN removes a key; rmx_clear_default_options() removes all. */
int rmx_set_default_option(const char* key, long value);
void rmx_clear_default_options(void);

/* The hot path.
 *   iq        complex64 interleaved I,Q  [n_windows][n_buoys][n_samples][2] float32, row-major
 *             (or uint8 with RMX_IN_U8); host pointer unless RMX_IN_DEVICE.
 *   pairs     int32 [n_pairs][2] = (i, j) buoy indices, or NULL for all i<j in nested-loop order
 *             (then n_pairs must be n_buoys*(n_buoys-1)/2 or 0).  Host pointer always.
 *   lag_int   int32   [n_windows][n_pairs]
 *   lag_frac  float32 [n_windows][n_pairs]   sub-sample offset in [-0.5, 0.5]
 *   peak      float32 [n_windows][n_pairs]   |c| at the integer peak (scipy scaling)
 * Range: everything is float32 with exact power-of-two scaling inside, so the level of the input is immaterial inside the
 * range: multiplying the window of any (window, buoy) by 2^e leaves lag_int and lag_frac bit-identical and multiplies peak
 * by 2^(e_i + e_j) exactly, on every route and for every request below (bounds, band, integration of groups at one level,
 * refinement, the Doppler search; the quality figures and all three outputs under PHAT do not move at all).
 * tests/test_gpu_dynamic_range.py holds every route to that bit for bit with e drawn per (window, buoy) from -20 ... +14
 * around rtl_sdr's +-127.5, i.e. from samples of 3e-5 rms to |sample| = 2.95e6.
 * The top: every route searches |c_s|^2 in float32, c_s = c / out_scale, and the largest |c| an input can produce is that
 * of a fully coherent window, N |sample|^2.  The squared magnitudes stay finite while
 *     |sample| < 2^32 sqrt(out_scale / N),
 * with out_scale = 2^5 at N = 4096 (k_win, k_fwd + k_pair), 2^4 at N = 8192 through k_win8kl, 2^3 at N = 16384 through
 * k16_fwd + k16_pairs, and 1 (log2 N odd) or 1/2 (log2 N even) through every other kernel at every length:
 *     N            16     64    256   1024   2048   4096   8192  16384  65536   2^18   2^20   2^22
 *     |sample| <  7.6e8  3.8e8  1.9e8  9.5e7  9.5e7  3.8e8  1.9e8  9.5e7  1.2e7  5.9e6  3.0e6  1.5e6
 *   (N = 4096, 8192 and 16384 through the generic kernels -- "generic4096", batches that k_win8kl / k16_* do not take --:
 *   4.7e7, 4.7e7 and 2.4e7; the lengths between follow the formula.)  Fully coherent windows (127.5 + 127.5j) 2^k are
 *   tested at the largest k below each bound and at k = 14 on every route.  Beyond the bound |c_s|^2 overflows and the
 *   outputs carry no meaning.
 *   integrate = K sums K squared magnitudes: divide the bound by K^(1/4).  The quality figures form the energy product
 *   (N |sample|^2)^2 and the fourth power of the stored spectra in float32: |sample| < 2^32 / sqrt(N) at every length
 *   (6.7e7 at N = 4096, 4.7e7 at 8192, 2.7e8 at 256).
 * The bottom: the three taps must stay normal float32 numbers, |c| / out_scale > 2^-63 at the peak and its neighbours;
 *   2^-20 x rtl_sdr's level on both buoys of a pair (|c|^2 near 2^-46 at N = 4096) is tested and exact.
 */
int rmx_xcorr_batch(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                    int32_t* lag_int, float* lag_frac, float* peak, unsigned flags);

/* rmx_xcorr_batch with the peak search restricted to a caller-given lag window per (window, pair): the physical
 * interval |lag| <= baseline / c + timing uncertainty of a TDoA pair, outside which every peak is false (an echo, a
 * co-channel transmitter, a periodic component, the wrap-around of a short window).
 *   lag_bounds  host int32 [lo, hi] in lag units (lag = k - (N-1)): [n_windows][n_pairs][2] when bounds_per_window is
 *               non-zero, else [n_pairs][2] shared by every window.  -(N-1) <= lo <= hi <= N-1, else RMX_E_INVAL (the
 *               window, pair and values in rmx_last_error).  The library copies the array through its own staging: the
 *               caller may reuse it as soon as the call returns, with RMX_OUT_DEVICE too.
 * Contract: S4-S6 above applied to the SLICE m[lo+N-1 .. hi+N-1] of the 'full' magnitude vector:
 *         k    = argmax over the slice (ties -> lowest k)   lag_int = k - (N-1), always in [lo, hi]
 *         lag_frac = the same parabola on m[k-1], m[k], m[k+1] when lo < lag_int < hi, and 0 when lag_int is lo or hi
 *         peak = m[k]
 *   with the same parity rules, computed on the slice (bit-exact lag_int wherever the oracle's top-two margin WITHIN the
 *   slice exceeds 1e-5; lowest index on exact ties; lag_frac within 1e-5 or the flat-peak bound).  The full interval
 *   [-(N-1), N-1] gives outputs bit-identical to rmx_xcorr_batch (a call whose every interval is the full one IS that
 *   call; a bounded call otherwise avoids the whole-window kernels g_win_* for N != 4096, 8192, 16384 -- batches of
 *   such N then run the per-transform kernels, whose float rounding of lag_frac may differ in the last bits).  Every other argument and flag means what it means
 *   there (RMX_IN_DEVICE, RMX_OUT_DEVICE, RMX_IN_U8, custom pair lists, chunking, the pipelined host-pointer path). */
int rmx_xcorr_batch_bounded(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                            const int32_t* lag_bounds, int bounds_per_window,
                            int32_t* lag_int, float* lag_frac, float* peak, unsigned flags);

/* weightings of rmx_xcorr_batch_weighted() */
enum { RMX_WEIGHT_NONE = 0, RMX_WEIGHT_PHAT = 1 };

/* Generalized cross-correlation: rmx_xcorr_batch (or rmx_xcorr_batch_bounded) on a band-limited and / or PHAT-whitened
 * cross-spectrum.  A band keeps one emitter of a wideband capture (two transmitters heard together otherwise share the
 * stronger one's lag); PHAT sets every bin to unit magnitude, so no single strong line -- the receivers' common DC offset
 * or LO leakage, which correlates at lag 0 -- dominates the peak.
 *   band_cps    NULL (every bin), or host double [lo, hi] in cycles per sample (f / fs): [n_windows][2] when
 *               band_per_window is non-zero (a window is one frequency group: its pairs share a band), else [2] shared
 *               by every window.  Finite, -0.5 <= lo <= hi <= 0.5; a band that wraps across +-fs/2 is not supported.
 *               Kept: the signed bins s in [-N, N-1] of the L = 2N point transform with lo <= s / L <= hi, i.e.
 *               s in [ceil(lo L), floor(hi L)] (exact: L is a power of two).  A band that keeps no bin (e.g. [0.5, 0.5])
 *               is RMX_E_INVAL, as is any other bad value; rmx_last_error names the window.
 *   weighting   RMX_WEIGHT_NONE or RMX_WEIGHT_PHAT; anything else is RMX_E_INVAL.
 *   lag_bounds  NULL, or exactly what rmx_xcorr_batch_bounded takes (the same sliced peak rule).
 * Definition: X_b = FFT_L(x_b zero padded) as in rmx_xcorr_batch;  Y_b[k] = M_w[k] X_b[k] (NONE) or
 *   M_w[k] X_b[k] / |X_b[k]| (PHAT; 0 where X_b[k] == 0: a dead receiver gives zeros, never NaN), M_w the 0/1 mask of
 *   window w's band;  r = IFFT_L(Y_j conj(Y_i)) with numpy's 1/L;  m[k] = |r[(k - (N-1)) mod L]|, k = 0 .. 2N-2;  then
 *   S4-S6 of rmx_xcorr_batch, or the sliced rule with lag_bounds.  peak = |r| at the integer peak.
 * Parity against a float32 restatement (tests/weighted_ref.py), with that helper's top-two margin inside the searched
 *   slice: lag_int bit-exact wherever the margin exceeds 1e-5; lag_frac within 1e-5 * max(|lag|, 1) or the flat-peak
 *   bound; peak within 1e-5 relative + 1e-6 of the vector's maximum.
 * No band (or the full one) with RMX_WEIGHT_NONE IS rmx_xcorr_batch / rmx_xcorr_batch_bounded: bit-identical outputs.
 * Otherwise the weight is applied where each forward spectrum is stored (it factors per buoy), so a weighted call runs the
 * per-transform kernels at every batch size -- k_fwd + k_pair at N = 4096, g_fwd_small + g_pair_small up to
 * L = small_maxl, the four-step kernels beyond -- never the whole-window ones (k_win, k_win8kl, k16_*, g_win_*,
 * g_rows_fused).  Every flag and the custom pair lists mean what they mean there.  The library copies the bands through
 * its own staging: the caller may reuse its arrays as soon as the call returns, with RMX_OUT_DEVICE too. */
int rmx_xcorr_batch_weighted(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                             const double* band_cps, int band_per_window, unsigned weighting,
                             const int32_t* lag_bounds, int bounds_per_window,
                             int32_t* lag_int, float* lag_frac, float* peak, unsigned flags);

/* Several bands per window over ONE set of forward spectra: every window is correlated under n_bands bands -- one per
 * emitter heard in the capture -- for B + n_bands P transforms and one upload of the samples, where n_bands repeated
 * windows through rmx_xcorr_batch_weighted cost n_bands (B + P) transforms and n_bands times the input bytes.
 *   band_cps    host double [lo, hi] in cycles per sample: [n_windows][n_bands][2] when bands_per_window is non-zero, else
 *               [n_bands][2] shared by every window.  Never NULL.  Every band obeys rmx_xcorr_batch_weighted's rules
 *               (finite, -0.5 <= lo <= hi <= 0.5, keeps at least one bin; no wrap across +-fs/2).
 *   n_bands     1 .. 64.
 *   weighting, lag_bounds, bounds_per_window   exactly as in rmx_xcorr_batch_weighted.  The bounds are per (window, pair)
 *               and shared by that window's bands: they come from the geometry, not from the emitter.
 *   lag_int, lag_frac, peak   [n_windows][n_bands][n_pairs].
 * Definition: slot (w, m, q) is slot (w, q) of rmx_xcorr_batch_weighted called with band[w][m] (band[m] when shared) and
 *   otherwise the same arguments: the same peak rule, sliced rule, parity statement (tests/bands_ref.py stacks
 *   tests/weighted_ref.py per band) and range statement.  The mask is a 0/1 weight, so it is applied where the product
 *   X_j conj(X_i) is formed instead of where the spectra are stored; the forward kernels run once per (window, buoy),
 *   unmasked (under PHAT: whitened), and the pair kernels walk n_bands virtual windows per window.
 *   It takes the per-transform kernels at every batch size, as the weighted call does; beyond L = small_maxl always the
 *   product-on-load inverse rows, never g_rows_anchor or g_rows_fused.
 * n_bands == 1 IS rmx_xcorr_batch_weighted with the same arguments: the same kernels, bit-identical outputs.
 * Refusals (RMX_E_INVAL, the text in rmx_last_error, nothing staged or written), in this order: a NULL buffer (band_cps
 *   included); n_bands outside 1 .. 64; rmx_xcorr_batch_weighted's weighting and band checks, the text naming the window and
 *   the band index; the batch shape (n_windows, pairs, n_pairs); rmx_xcorr_batch_bounded's checks.
 *   n_windows == 0 or n_pairs == 0 returns RMX_OK and writes nothing.
 * Every flag (RMX_IN_DEVICE, RMX_OUT_DEVICE, RMX_IN_U8), the custom pair lists and the chunking work as in
 * rmx_xcorr_batch_weighted.  The library copies the bands and the bounds through its own staging: the caller may reuse its
 * arrays as soon as the call returns, with RMX_OUT_DEVICE too.
 * There is no integration, refinement or quality here: rmx_xcorr_batch_bands sums over no windows, is not refined and
 * reports no quality. */
int rmx_xcorr_batch_bands(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                          const double* band_cps, int n_bands, int bands_per_window, unsigned weighting,
                          const int32_t* lag_bounds, int bounds_per_window,
                          int32_t* lag_int, float* lag_frac, float* peak, unsigned flags);

/* Noncoherent integration: rmx_xcorr_batch_weighted with ONE peak search per group of `integrate` consecutive windows,
 * on the lag-by-lag sum of the windows' squared correlation magnitudes.  Two receivers with free-running oscillators stay
 * phase-coherent over a short segment only (a frequency offset rotates the cross-spectrum and the coherent peak of a long
 * window collapses), and a weak emitter's single-window peak may lie below the largest noise lag; cutting the capture
 * into K short windows and summing |c|^2 over them repairs both, without a Doppler search.
 *   integrate   K >= 1 windows per group.  n_windows must be a positive multiple of K; windows g K .. g K + K - 1 form
 *               group g, G = n_windows / K groups.  Anything else is RMX_E_INVAL (the values in rmx_last_error).
 *   band_cps, band_per_window, weighting   exactly as in rmx_xcorr_batch_weighted: bands stay per WINDOW ([n_windows][2] or [2]).
 *   lag_bounds  NULL, or host int32 [lo, hi]: [G][n_pairs][2] when bounds_per_group is non-zero, else [n_pairs][2] shared
 *               by every group; the sliced rule of rmx_xcorr_batch_bounded, applied to m below.
 *   lag_int / lag_frac / peak   [G][n_pairs] (not [n_windows][n_pairs]).
 * Definition, for group g and pair (i, j): c_w = the correlation of window w exactly as rmx_xcorr_batch_weighted defines
 *   it (band mask and PHAT where given);  s[k] = sum over the group's windows, in window order, of |c_w[k]|^2 in float32;
 *   m[k] = sqrt(s[k]) (scipy scaling: the root-sum-square of the per-window magnitudes);  then S4-S6 of rmx_xcorr_batch on
 *   m -- argmax with the lowest index on ties, the parabola on m[k-1], m[k], m[k+1], peak = m[k] -- or the sliced rule
 *   with lag_bounds.  The kernels search the maximum of s and take the square root of the three taps only; the note on
 *   that at rmx_xcorr_batch applies unchanged.  The additions of a lag's K terms are made by one thread in window order:
 *   two identical calls give bit-identical outputs.
 * Parity against a float32 restatement (tests/integrated_ref.py) is that of rmx_xcorr_batch_weighted, computed on m; the
 *   in-order float32 sum of K positive terms adds at most (K - 1) 2^-24 relative (4e-6 at K = 64).
 * integrate == 1 IS rmx_xcorr_batch_weighted with the same arguments: bit-identical outputs.
 * Otherwise the call runs the per-transform kernels at every batch size, like a weighted call -- k_fwd + k_pair (the
 * streaming variant) at N = 4096, g_fwd_small + g_pair_small up to L = small_maxl, the four-step kernels beyond, for every
 * N rmx_create accepts -- never the whole-window ones.  The forward kernels run on all windows; the pair / peak kernels
 * run one work item per (group, pair) that walks the group's windows (radio-mapper_amd/csrc/integrate.hpp).  Flags,
 * custom pair lists and chunking mean what they mean for the weighted entry.  A chunk always holds whole groups: K larger
 * than the largest chunk the ctx can hold (option "chunk_windows" at N = 4096, the scratch budget elsewhere) is
 * RMX_E_INVAL with a text that says so, never a silent split. */
int rmx_xcorr_batch_integrated(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                               int integrate,
                               const double* band_cps, int band_per_window, unsigned weighting,
                               const int32_t* lag_bounds, int bounds_per_group,
                               int32_t* lag_int, float* lag_frac, float* peak, unsigned flags);

/* Fine lag search: rmx_xcorr_batch_integrated with the sub-sample estimate taken from the band-limited interpolant of the
 * SAME correlation on a grid of 1 / U samples around the integer peak, instead of a parabola through three integer lags.
 * The peak of a band-limited correlation is a sinc (a Dirichlet kernel under PHAT), not a parabola: the three-point fit
 * carries a deterministic bias of up to 0.15 samples (0.06 rms at bandwidth 0.8 fs, 0.25 on a white source) that neither
 * averaging nor a longer window removes.  On the fine grid the same parabola spans 2 / U samples and the bias falls to
 * 0.002 ... 0.015 samples rms at 10 dB.  A narrow band (0.2 fs or less) is noise-limited:
 * refinement gains nothing there.
 *   refine      U, one of 0, 2, 4, 8, 16; anything else is RMX_E_INVAL with the value in rmx_last_error (refused after the
 *               integrate, weighting / band and lag_bounds checks, before anything is copied).
 *   every other argument means exactly what it means for rmx_xcorr_batch_integrated.
 * Definition, for one (window, pair) -- or one (group, pair) of an integrated call: lag0 is the integer lag the existing
 *   rule finds, unchanged, searched in [lo, hi] (the full interval [-(N-1), N-1] without lag_bounds).  With Y_b the
 *   (weighted) L = 2N point spectra exactly as rmx_xcorr_batch_weighted defines them:
 *     P[s]  = Y_j[s mod L] * conj(Y_i[s mod L])         signed bins s = -N .. N-1
 *     r(t)  = (1/L) * sum_s P[s] * exp(+2*pi*i*s*t/L)   real t; r at integer t is the existing r[t mod L]
 *     f[u]  = |r(lag0 + u/U)|                           integer u in [-U, U] with lo <= lag0 + u/U <= hi
 *             integrated call: f[u] = sqrt( sum over the group's windows, in window order, of |r_w(lag0 + u/U)|^2 )
 *     u*    = the admitted u with the largest f; equal values: the smallest |u|, then the negative one
 *             (so an all-zero window gives u* = 0)
 *     d     = the S5 parabola on f[u*-1], f[u*], f[u*+1], in double from the float32 taps;
 *             0 when a neighbour is not admitted, or when the denominator is 0
 *     delta = (u* + d) / U
 *     n     = +1 if delta > 0.5, -1 if delta < -0.5, else 0
 *     lag_int  = lag0 + n        (inside [lo, hi] by construction)
 *     lag_frac = (float)(delta - n)   in [-0.5, 0.5]
 *     peak     = f[u*]
 *   The fine rule never changes which integer peak was chosen; it relocates the estimate within +-1 sample of it.
 * Parity against a float64 restatement (tests/refined_ref.py), where that restatement's coarse top-two margin exceeds
 *   1e-5: lag_int + lag_frac within 1e-5 * max(|lag|, 1) or the flat-peak bound of the fine taps divided by U (the two
 *   parts may split differently near delta = +-0.5); peak within 1e-5 relative + 1e-6 of the vector's maximum.
 * refine == 0 IS rmx_xcorr_batch_integrated with the same arguments: bit-identical outputs, the same kernels.
 * Otherwise both spectra of a pair must be in HBM, so the call runs the per-transform kernels at every batch size, exactly
 *   as a weighted call does (a full band and no whitening when the caller gave none), and one more kernel, k_refine
 *   (radio-mapper_amd/csrc/refine.hpp), runs behind each chunk's pair kernels: it reads lag0 from the outputs, sums the
 *   cross-spectrum in storage order with exact rational phases, reduces in a fixed tree (two identical calls give
 *   bit-identical outputs) and overwrites the three outputs in place.  (The Doppler search: rmx_caf_batch_quality.) */
int rmx_xcorr_batch_refined(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                            int integrate,
                            const double* band_cps, int band_per_window, unsigned weighting,
                            const int32_t* lag_bounds, int bounds_per_group, int refine,
                            int32_t* lag_int, float* lag_frac, float* peak, unsigned flags);

/* the four values of one output slot of rmx_xcorr_batch_quality(): quality[slot][RMX_Q_...] */
enum { RMX_Q_COHERENCE = 0, RMX_Q_PSR = 1, RMX_Q_RMS_BW = 2, RMX_Q_NEFF = 3 };

/* Qualified lags: rmx_xcorr_batch_refined with four figures per output slot that say whether its lag can be trusted.
 * `peak` is in scipy's scaling -- it grows with the window length and the input power, so it cannot be thresholded, and
 * a noise-only window yields a lag exactly as a 20 dB emitter does.  The figures below are normalised.
 *   quality     float32 [rows][n_pairs][4], rows = n_windows, or the G groups of an integrated call; a device pointer
 *               with RMX_OUT_DEVICE, like the other three outputs.  NULL: the call IS rmx_xcorr_batch_refined.  It must
 *               not overlap lag_int, lag_frac or peak (RMX_E_INVAL naming the array; refused after the integrate,
 *               weighting / band, lag_bounds and refine checks, before anything is copied).
 *   every other argument means exactly what it means for rmx_xcorr_batch_refined.
 * Definition, for one output slot -- (window, pair), or (group g, pair) of an integrated call with its K windows w in
 *   window order -- and pair (i, j); Y_b,w the (weighted) L = 2N point spectra exactly as rmx_xcorr_batch_weighted
 *   defines them, s the signed bin of k (s = k, or k - L for k >= N):
 *     A_w = sum_k |Y_i,w[k]|^2            B_w = sum_k |Y_j,w[k]|^2
 *     C_w = sum_k |Y_i,w[k]|^2 |Y_j,w[k]|^2          (= sum |P|^2,  P = Y_j conj(Y_i))
 *     D_w = sum_k |Y_i,w[k]| |Y_j,w[k]|              (= sum |P|)
 *     F_w = sum_k (s / L)^2 |Y_i,w[k]| |Y_j,w[k]|
 *     EE  = sum_w (A_w / L) (B_w / L)     the energy product of the two windows (time domain, by Parseval)
 *     Et  = sum_w C_w / L                 = sum_w sum over ALL L circular lags of |r_w|^2 (Parseval on r = IFFT_L(P))
 *     p0  = the COARSE rule's peak of this slot (m[k*]; sqrt(s[k*]) when integrated), before any refinement
 *   quality[RMX_Q_COHERENCE] = min(p0 / sqrt(EE), 1); 0 when EE = 0.  The normalised correlation coefficient in [0, 1]
 *       (Cauchy-Schwarz per window); 1 for identical windows; under PHAT p0 L / (kept bins).
 *   quality[RMX_Q_PSR]       = p0^2 (L - 1) / (Et - p0^2); +inf when the denominator <= 0 < p0; 0 when p0 = 0.  The peak
 *       power over the mean power of all OTHER circular lags.  For a white noise-only pair each |r[k]|^2 / floor is
 *       Exp(1) -- Gamma(K) / K when K windows are integrated --, but the zero-padded linear correlation has a triangular
 *       variance, up to 2 x the mean floor near lag 0: a threshold for a false-alarm rate must allow for that factor
 *       (xcorr.psr_threshold does).
 *   quality[RMX_Q_RMS_BW]    = sqrt(sum_w F_w / sum_w D_w) cycles per sample; 0 when sum D = 0.  The rms bandwidth of the
 *       cross-spectrum, which sets the peak's curvature.
 *   quality[RMX_Q_NEFF]      = (sum_w D_w)^2 / sum_w C_w; 0 when sum C = 0.  The participation count of bins (a
 *       time-bandwidth product): L under full-band PHAT, K L when K windows are integrated.
 *   A dead receiver (all zeros) gives four zeros, never NaN.
 * The sums run over the stored float32 spectra in storage order, five float32 partial sums per thread and window,
 *   reduced in a fixed tree and added over the windows in window order: two identical calls give bit-identical outputs.
 * Parity against a float64 restatement (tests/quality_ref.py): coherence, rms_bw and n_eff within 1e-4 relative;
 *   psr compared as Et / p0^2 = (L - 1) / psr + 1 within 1e-4 relative (the difference Et - p0^2 cancels on a clean
 *   signal).
 * quality == NULL IS rmx_xcorr_batch_refined with the same arguments: bit-identical outputs, the same kernels.
 * lag_int, lag_frac and peak of a quality call are bit-identical to the same call without quality, whatever route that
 *   call takes; k_quality (radio-mapper_amd/csrc/quality.hpp) writes nothing but quality.  Both spectra of a pair must be
 *   in HBM for it, so:
 *   - a call with a band, a weighting, integration or refinement runs the per-transform kernels at every batch size
 *     anyway, and k_quality runs behind each chunk's pair kernels and in front of k_refine, which overwrites peak;
 *   - a call with none of those first runs exactly what the call without quality runs (the whole-window kernels k_win,
 *     k_win8kl, k16_*, g_win_*, g_rows_fused included, which keep their spectra to themselves and round lag_frac and
 *     peak differently in the last bits than the per-transform kernels), then, chunk by chunk, the per-transform
 *     forward kernels and k_quality: one more forward pass, and the outputs stay those of the call without quality.
 *   (The Doppler search: rmx_caf_batch_quality.) */
int rmx_xcorr_batch_quality(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                            int integrate,
                            const double* band_cps, int band_per_window, unsigned weighting,
                            const int32_t* lag_bounds, int bounds_per_group, int refine,
                            int32_t* lag_int, float* lag_frac, float* peak, float* quality, unsigned flags);

/* Refined and qualified lags of several bands per window: rmx_xcorr_batch_bands with the fine lag search of
 * rmx_xcorr_batch_refined and the four figures of rmx_xcorr_batch_quality per (window, band, pair), still over ONE set of
 * forward spectra per window.
 *   band_cps, n_bands, bands_per_window, weighting, lag_bounds, bounds_per_window   exactly as in rmx_xcorr_batch_bands.
 *   refine      U, one of 0, 2, 4, 8, 16, as in rmx_xcorr_batch_refined.
 *   lag_int, lag_frac, peak   [n_windows][n_bands][n_pairs].
 *   quality     float32 [n_windows][n_bands][n_pairs][4] (RMX_Q_...), or NULL; a device pointer with RMX_OUT_DEVICE.  It
 *               must not overlap lag_int, lag_frac or peak.
 * Definition: slot (w, m, q) is slot (w, q) of rmx_xcorr_batch_quality called with integrate = 1, band[w][m] (band[m] when
 *   shared) and otherwise the same arguments -- all four outputs, and that entry's parity statements (tests/
 *   bands_quality_ref.py stacks tests/refined_ref.py and tests/quality_ref.py per band).  There is no integration here:
 *   rmx_xcorr_batch_bands_integrated is this entry with `integrate`.
 * refine == 0 and quality == NULL IS rmx_xcorr_batch_bands: the same kernels, bit-identical outputs.
 * n_bands == 1 IS rmx_xcorr_batch_quality with integrate = 1 and the same arguments, bit-identical.
 * Otherwise the call runs exactly what rmx_xcorr_batch_bands runs -- one forward pass, the banded pair kernels -- and
 *   behind each chunk's pair kernels the banded instantiations k_quality<layout, BandSet>, then k_refine<U, layout,
 *   BandSet> (radio-mapper_amd/csrc/quality.hpp, refine.hpp): one workgroup per (virtual window, pair) reads the real
 *   window's two unmasked spectra and skips every stored position whose bin the slot's band drops.  Those positions are
 *   stored zeros in the weighted call and add +-0 there, so away from the four-step route with the default pair list from
 *   6 buoys on (where the weighted call's coarse peak comes from g_rows_anchor) slot (w, m, q) is bit-identical to
 *   rmx_xcorr_batch_quality with band[w][m].  lag_int, lag_frac and peak of a call with quality
 *   are bit-identical to the same call without it.
 * Refusals (RMX_E_INVAL, the text in rmx_last_error, nothing staged or written), in this order: rmx_xcorr_batch_bands' own,
 *   in its order; refine not one of 0, 2, 4, 8, 16; quality overlapping another output, the text naming the array.
 *   n_windows == 0 or n_pairs == 0 returns RMX_OK and writes nothing.
 * Flags, custom pair lists, chunking and the staging of bands and bounds work as in rmx_xcorr_batch_bands. */
int rmx_xcorr_batch_bands_quality(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                                  const double* band_cps, int n_bands, int bands_per_window, unsigned weighting,
                                  const int32_t* lag_bounds, int bounds_per_window, int refine,
                                  int32_t* lag_int, float* lag_frac, float* peak, float* quality, unsigned flags);

/* Noncoherent integration under several bands per window: rmx_xcorr_batch_bands_quality plus `integrate`, for captures
 * that hold several emitters AND come from free-running receivers or weak emitters.  ONE set of forward spectra per window
 * serves every band and every group.
 *   integrate   K >= 1; n_windows must be a positive multiple of K: G = n_windows / K groups of consecutive windows, as in
 *               rmx_xcorr_batch_integrated.
 *   band_cps    stays per WINDOW: float64 [n_windows][n_bands][2], or [n_bands][2] shared (bands_per_window == 0).  The
 *               windows of one group may carry different bands in column m.
 *   lag_bounds  NULL, int32 [n_pairs][2] (bounds_per_group == 0), or [G][n_pairs][2] per group; shared by the group's bands.
 *   lag_int, lag_frac, peak   [G][n_bands][n_pairs].
 *   quality     float32 [G][n_bands][n_pairs][4] (RMX_Q_...), or NULL.  It must not overlap lag_int, lag_frac or peak.
 * Definition: slot (g, m, q) is slot (g, q) of rmx_xcorr_batch_quality called with the same integrate, weighting, lag_bounds
 *   and refine, band_per_window = 1 and band[w] = band_cps[w][m] (band_cps[m] when shared) -- all four outputs, that entry's
 *   parity statements unchanged, and its (K - 1) 2^-24 note on the in-order sum (tests/bands_integrated_ref.py stacks
 *   tests/integrated_ref.py, refined_ref.py and quality_ref.py per band).
 * integrate == 1 IS rmx_xcorr_batch_bands_quality; n_bands == 1 IS rmx_xcorr_batch_quality; refine == 0, quality == NULL and
 *   integrate == 1 IS rmx_xcorr_batch_bands: each the same kernels, bit-identical outputs.  lag_int, lag_frac and peak of a
 *   call with quality are bit-identical to the same call without it.
 * Otherwise the forward kernels run once per (window, buoy) on all windows -- unmasked, or under PHAT whitened with the
 *   full band -- and the pair kernels run in their banded integrating instantiations, pack <LagBounds, Integrate, BandSet>
 *   (radio-mapper_amd/csrc/xspec_bands.hpp): a work item is (group, band, pair); it walks the group's real windows, masks
 *   each window's product with band (window, m) and adds |r|^2 into per-thread accumulators in window order, then searches
 *   the peak once.  k_quality and k_refine follow in the same pack.  A dropped bin is a stored +0 in the single-band call and
 *   a skipped +0 here, and the K terms of a lag are added by one thread in window order on both sides, so away from the
 *   four-step route with the default pair list from 6 buoys on (where the single-band integrated call's coarse peak comes
 *   from g_rows_anchor, which the banded call never takes) slot (g, m, q) is bit-identical to rmx_xcorr_batch_quality with
 *   band m; there the slot is held to the reference's bars.
 * Refusals (RMX_E_INVAL, the text in rmx_last_error, nothing staged or written), in this order: integrate < 1, or n_windows
 *   not a positive multiple of it; a NULL buffer (band_cps included); a misaligned device pointer; n_bands outside 1..64;
 *   the weighting and the bands, the text naming band m of the REAL window w; the batch shape; the bounds, the text saying
 *   "group" when integrate > 1; refine; quality overlapping another output.  Then the route: a chunk holds whole groups AND
 *   at most the virtual windows and bytes the bands allow -- a K that no such chunk holds is refused, the text naming K,
 *   n_bands and the chunk the bands left; never a silent split of a group.  RMX_E_UNSUPPORTED for the column tile of
 *   rmx_xcorr_batch_integrated.
 * Flags, custom pair lists and the staging of bands and bounds work as in rmx_xcorr_batch_bands. */
int rmx_xcorr_batch_bands_integrated(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                                     int integrate,
                                     const double* band_cps, int n_bands, int bands_per_window, unsigned weighting,
                                     const int32_t* lag_bounds, int bounds_per_group, int refine,
                                     int32_t* lag_int, float* lag_frac, float* peak, float* quality, unsigned flags);

/* Cross-ambiguity variant of the hot path (BASELINE configs[4]): for
 * every window and pair (i, j) the later buoy's window is de-rotated by each Doppler hypothesis,
 *     c_d = correlate(x[w][j] * exp(-2*pi*i*doppler_cps[d]*n), x[w][i], 'full', 'fft'),
 * and the peak is searched over (d, lag) in d-major order (ties -> lowest d, then lowest lag index);
 * the lag is interpolated along the lag axis of the winning row exactly as in rmx_xcorr_batch.
 *   doppler_cps  host array [n_dopplers], cycles per sample (f_d / fs)
 *   dop_idx      int32 [n_windows][n_pairs]  index of the winning hypothesis
 * Same buffer/flag conventions as rmx_xcorr_batch.  The reference has no counterpart (its TDoA is a
 * timestamp subtraction, tdoa_processor.py:166); the oracle is oracle/xcorr_ref.py:caf_pair. */
int rmx_caf_batch(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                  const double* doppler_cps, int n_dopplers, int32_t* dop_idx, int32_t* lag_int,
                  float* lag_frac, float* peak, unsigned flags);

/* The Doppler search with the per-call request of the correlation entries -- a band, PHAT, lag bounds -- and a sub-grid
 * Doppler estimate.  Free-running receivers that differ by hundreds of hertz are also the ones with a common DC offset,
 * LO leakage and echoes; the DC offset correlates at lag 0 and nu = 0, and a search over D hypotheses gives it D times
 * as many chances to win.  PHAT, or a band that leaves out DC, repairs that.
 *   band_cps, band_per_window, weighting   exactly as in rmx_xcorr_batch_weighted ([n_windows][2] or [2]; shared by all hypotheses).
 *   lag_bounds, bounds_per_window          exactly as in rmx_xcorr_batch_bounded, or NULL; the interval of a (window, pair)
 *               is shared by all its hypotheses.
 *   dop_frac    float32 [n_windows][n_pairs], a device pointer with RMX_OUT_DEVICE; NULL: not computed.  The offset of the
 *               Doppler estimate from doppler_cps[dop_idx], in grid INDICES: it presumes a uniformly spaced grid
 *               (xcorr.doppler_estimate turns it into cycles per sample and refuses other grids).  It must not overlap
 *               one of the other four outputs.
 * Definition, for window w, pair (i, j) and hypothesis d:
 *     Y_i   = weight_w(FFT_L(x_i))                 Y_j,d = weight_w(FFT_L(x_j * rot_d))
 *   with rot_d the phasor table of rmx_caf_batch and weight_w the band mask and PHAT of rmx_xcorr_batch_weighted, applied
 *   to the stored spectrum of each transform, after the rotation;  r_d = IFFT_L(Y_j,d conj(Y_i)), m_d its 'full' magnitudes.
 *   Per hypothesis S4-S6 of rmx_xcorr_batch on m_d -- the sliced rule of rmx_xcorr_batch_bounded with lag_bounds -- give
 *   (lag_d, frac_d, peak_d); dop_idx = d* is the d-major first maximum of peak_d (strict >: ties keep the lowest d), and
 *   lag_int, lag_frac, peak are lag_d*, frac_d*, peak_d*.
 *     dop_frac = (float)((a - c) / (2 (a - 2 b + c))) in double, a, b, c = the float32 peak_d of d* - 1, d*, d* + 1;
 *     dop_frac = 0 when d* is 0 or n_dopplers - 1.
 *   The first-maximum rule gives a < b and c <= b: the denominator is negative and dop_frac lies in (-0.5, 0.5].
 * rmx_caf_batch IS this call with no band, RMX_WEIGHT_NONE, no bounds and dop_frac == NULL: the same kernels, bit-identical
 *   outputs.  A full band with RMX_WEIGHT_NONE and full-interval bounds is that plain call too.  A non-NULL dop_frac changes
 *   nothing in the other four outputs.
 * Refusals (RMX_E_INVAL, the text in rmx_last_error, nothing written): the checks of rmx_caf_batch, then those of the
 *   weighted entry, then those of the bounded entry, then dop_frac overlapping another output.
 * The routes are rmx_caf_batch's: every weighted or bounded instantiation runs where the plain one runs, with the same
 *   launch counts (the N = 4096 one-launch path included); a non-NULL dop_frac swaps k_caf_select(_all) for
 *   k_caf_select(_all)_fd (radio-mapper_amd/csrc/caf_select.hpp).
 * There is no integration here.  Refinement and quality: rmx_caf_batch_quality, which this entry is with neither; the
 * search integrated over groups of windows: rmx_caf_batch_integrated. */
int rmx_caf_batch_request(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                          const double* doppler_cps, int n_dopplers,
                          const double* band_cps, int band_per_window, unsigned weighting,
                          const int32_t* lag_bounds, int bounds_per_window,
                          int32_t* dop_idx, float* dop_frac,
                          int32_t* lag_int, float* lag_frac, float* peak, unsigned flags);

/* Refined and qualified lags of the Doppler search: rmx_caf_batch_request with the fine lag search of
 * rmx_xcorr_batch_refined and the four figures of rmx_xcorr_batch_quality on each slot's WINNING hypothesis.  Receivers
 * whose oscillators differ by hundreds of hertz are the ones whose lags most need a threshold (quality[RMX_Q_PSR] against
 * xcorr.psr_threshold) and a weight for rmx_solve_batch (xcorr.lag_sigma).
 *   refine      U, one of 0, 2, 4, 8, 16, as in rmx_xcorr_batch_refined.
 *   quality     float32 [n_windows][n_pairs][4] (RMX_Q_...), or NULL; a device pointer with RMX_OUT_DEVICE.  It must not
 *               overlap one of the five other outputs.
 *   every other argument means exactly what it means for rmx_caf_batch_request.
 * Definition, for window w, pair (i, j) and the winner d* = dop_idx[w][q]:
 *   The winner is chosen exactly as in rmx_caf_batch_request, on the coarse per-hypothesis peaks, and is never revisited:
 *   dop_idx and dop_frac do not move when refine or quality is set, and dop_frac stays the parabola through the COARSE peaks.
 *   lag_int, lag_frac, peak and quality of the slot are those of rmx_xcorr_batch_quality for the pair of windows
 *   (x_i, x_j * rot_d*) with integrate = 1 and this call's band, weighting, lag bounds and refine:
 *     Y_i and Y_j,d* are the weighted un-rotated and de-rotated spectra exactly as rmx_caf_batch_request defines them (the
 *       weight applied to the stored spectrum after the rotation);
 *     lag0 and p0 are the winner's coarse lag and coarse peak (lag_d*, peak_d*);
 *     quality is computed with p0, before any refinement;
 *     refine then overwrites lag_int, lag_frac and peak by the rule of rmx_xcorr_batch_refined.
 *   Parity against a float64 restatement (tests/caf_quality_ref.py stacks tests/caf_request_ref.py, refined_ref.py and
 *   quality_ref.py on the winner's rotated pair): the bars of rmx_xcorr_batch_refined and rmx_xcorr_batch_quality.
 * refine == 0 and quality == NULL IS rmx_caf_batch_request: the same kernels, the same launches, bit-identical outputs.
 *   With refine == 0, lag_int, lag_frac and peak are bit-identical to the call without quality.
 * Otherwise the search itself runs exactly what rmx_caf_batch_request runs, and behind the selection k_quality<layout,
 *   CafWinner>, then k_refine<U, layout, CafWinner> (radio-mapper_amd/csrc/caf_select.hpp, quality.hpp, refine.hpp) read
 *   operand i from the un-rotated spectra and operand j from the winner's de-rotated ones.  Under a band the spectra are
 *   stored masked, so these are the plain kernel bodies.
 *   - The one-launch path of N = 4096 holds every hypothesis' spectra when the selection has run: one launch of each
 *     kernel, slot (w, q) reading operand j at virtual window dop_idx * n_windows + w; no transform is added.
 *   - Every other route overwrites hypothesis d's spectra with d + 1's and knows the winner only after the last one:
 *     behind the last hypothesis of each chunk the hypotheses are swept a second time, each forward pass followed by the
 *     two kernels, whose workgroups return at once unless dop_idx[slot] == d.  n_dopplers more forward launches and
 *     n_dopplers launches of each kernel per chunk; no scratch.
 * Refusals (RMX_E_INVAL, the text in rmx_last_error, nothing staged or written), in this order: rmx_caf_batch_request's own,
 *   in its order; refine not one of 0, 2, 4, 8, 16, with the value; quality overlapping one of the five other outputs, the
 *   text naming the array; a device quality not aligned to 4 bytes.  n_windows == 0 or n_pairs == 0 returns RMX_OK and
 *   writes nothing.
 * There is no integration here.  rmx_caf_batch_integrated is this entry with `integrate`. */
int rmx_caf_batch_quality(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                          const double* doppler_cps, int n_dopplers,
                          const double* band_cps, int band_per_window, unsigned weighting,
                          const int32_t* lag_bounds, int bounds_per_window, int refine,
                          int32_t* dop_idx, float* dop_frac,
                          int32_t* lag_int, float* lag_frac, float* peak, float* quality, unsigned flags);

/* The Doppler search integrated noncoherently over consecutive windows: coherent inside each window under a frequency
 * hypothesis, noncoherent across the K windows of a group -- the weak-signal form for receivers with free-running
 * oscillators.  rmx_xcorr_batch_integrated alone fails once the offset reaches one cycle per window (every term of its
 * sum then sits on the null of the window's own sinc); rmx_caf_batch_quality alone has no processing gain beyond one
 * window.  Here every hypothesis is de-rotated per window and |r|^2 is summed over the group before ONE peak search.
 *   integrate   K >= 1; n_windows must be a positive multiple of K: G = n_windows / K groups of K consecutive windows, as
 *               in rmx_xcorr_batch_integrated.
 *   band_cps, band_per_window, weighting   stay per WINDOW ([n_windows][2] or [2]), shared by all hypotheses.
 *   lag_bounds  NULL, host int32 [n_pairs][2] (bounds_per_group == 0), or [G][n_pairs][2] per group; the interval of a
 *               (group, pair) is shared by all its hypotheses.
 *   dop_idx, dop_frac (or NULL), lag_int, lag_frac, peak   [G][n_pairs];  quality  float32 [G][n_pairs][4], or NULL.
 *   every other argument means exactly what it means for rmx_caf_batch_quality.
 * Definition, for group g, pair (i, j) and hypothesis d:
 *     r_{w,d}  = the per-window correlation of rmx_caf_batch_request, exactly: the same phasor table rot_d, indexed
 *                n = 0 .. N-1 in EVERY window (the phase origin of a window is immaterial under |.|^2), the band mask and
 *                PHAT of window w on each stored spectrum after the rotation;
 *     s_d[k]   = sum over the group's windows, in window order, of |r_{w,d}[k]|^2, in float32, by one thread;
 *     m_d[k]   = sqrt(s_d[k]);
 *   per hypothesis S4-S6 of rmx_xcorr_batch on m_d -- the sliced rule of rmx_xcorr_batch_bounded on the group's interval --
 *   give (lag_d, frac_d, peak_d); dop_idx = d* is the d-major first maximum of peak_d (strict >: ties keep the lowest d);
 *   dop_frac is rmx_caf_batch_request's parabola through the integrated peak_d of d* - 1, d*, d* + 1.  The winner is never
 *   revisited.
 *   refine and quality are those of rmx_xcorr_batch_quality with the same `integrate`, computed on the window sequences
 *   (x_{i,w}, x_{j,w} * rot_d*) of the group: quality uses the coarse integrated peak p0 = peak_d*; refine then
 *   overwrites lag_int, lag_frac and peak by the rule of rmx_xcorr_batch_refined (f[u] summed over the group's windows).
 *   Parity against a float restatement (tests/caf_integrated_ref.py stacks tests/caf_request_ref.py, integrated_ref.py,
 *   refined_ref.py and quality_ref.py): the bars of rmx_caf_batch_quality and rmx_xcorr_batch_integrated, with that
 *   entry's (K - 1) 2^-24 note on the in-order sum; dop_idx and lag_int exact where the restatement's hypothesis margin
 *   and top-two lag margin, both taken on the integrated vectors, exceed 1e-5.
 * Range: the sum of K windows' |r|^2 is K times as large as one window's: divide the |sample| bound of rmx_xcorr_batch by
 *   K^(1/4), as for rmx_xcorr_batch_integrated.
 * integrate == 1 IS rmx_caf_batch_quality with the same arguments (one checked request behind both): the same kernels, the same
 *   launches, bit-identical outputs.  With refine == 0 and quality == NULL nothing is launched behind the selection;
 *   lag_int, lag_frac and peak of a call with quality are bit-identical to the same call without it.  A call whose
 *   hypotheses are applied to buoy j's windows on the host (the same float32 phasors) and that goes through
 *   rmx_xcorr_batch_quality with the same integrate and request gives, at the coarse first maximum, the same bits.
 * Otherwise the forward kernels are those of the search, on all windows, and every route of rmx_caf_batch_quality takes
 *   the call with its integrating pair kernels reading operand j from the de-rotated set: the pack <LagBounds, Integrate,
 *   CafOperand> of k_pair_str and g_pair_small (radio-mapper_amd/csrc/integrate.hpp); the four-step row kernels take the
 *   second operand set as they are and g_cols_inv's integrating instantiation sums their products (never g_rows_fused).
 *   - N = 4096, every hypothesis in one launch (the condition is rmx_caf_batch's, on n_windows): two forward launches, ONE
 *     integrating pair launch over n_dopplers * G virtual groups gv = d * G + g (operand j at virtual windows gv * K + kw,
 *     operand i and the lag interval at real group g), the selection over [n_dopplers][G][n_pairs], then at most one
 *     k_quality and one k_refine launch.
 *   - N = 4096 in chunks, the small route, the four-step route: chunks are rounded down to whole groups; per hypothesis
 *     forward, the integrating pair kernels, k_caf_select(_fd) on the chunk's G' * n_pairs slots; then, with refine or
 *     quality, the second sweep of rmx_caf_batch_quality, whose workgroups walk their group's K windows.
 * Refusals (RMX_E_INVAL, the text in rmx_last_error, nothing staged or written), in this order: rmx_caf_batch_quality's
 *   head (a NULL buffer, a misaligned device pointer, n_dopplers); integrate < 1, or n_windows not a positive multiple of
 *   it (the values in the text; integrate == 1 takes an empty batch as rmx_caf_batch_quality does); the batch shape and
 *   the pair list; the weighting and the bands, the text naming the real window; the bounds, the text saying "group" when
 *   integrate > 1; dop_frac overlapping another output; refine; quality overlapping another output or misaligned -- every
 *   extent G * n_pairs slots; then the route: a chunk holds whole groups, and a K that no chunk of the ctx holds (option
 *   "chunk_windows" at N = 4096, the scratch budget elsewhere) is refused with a text that says so, never a silent
 *   split.  RMX_E_UNSUPPORTED for the column tile of rmx_xcorr_batch_integrated.
 * Several bands under the search: rmx_caf_batch_bands, which has no integration. */
int rmx_caf_batch_integrated(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                             const double* doppler_cps, int n_dopplers, int integrate,
                             const double* band_cps, int band_per_window, unsigned weighting,
                             const int32_t* lag_bounds, int bounds_per_group, int refine,
                             int32_t* dop_idx, float* dop_frac,
                             int32_t* lag_int, float* lag_frac, float* peak, float* quality, unsigned flags);

/* The Doppler search under several bands per window over ONE set of forward passes: rmx_caf_batch_request for a capture
 * that holds several emitters, each in its own band, heard by receivers with free-running oscillators.  The forward
 * transforms do not depend on the band: (1 + n_dopplers) * n_buoys of them per window serve all n_bands bands, where
 * n_bands calls of rmx_caf_batch_request run n_bands times as many, and the windows are uploaded once.
 *   band_cps, n_bands (1 .. 64), bands_per_window   exactly as in rmx_xcorr_batch_bands ([n_windows][n_bands][2] or
 *               [n_bands][2]; never NULL); the bands of a window are shared by all its hypotheses.
 *   doppler_cps, n_dopplers, weighting, lag_bounds, bounds_per_window, dop_frac (or NULL), flags
 *               exactly as in rmx_caf_batch_request.  The bounds are per (window, pair), shared by the window's bands and
 *               hypotheses.
 *   dop_idx, dop_frac, lag_int, lag_frac, peak   [n_windows][n_bands][n_pairs].
 * Definition: slot (w, m, q) is slot (w, q) of rmx_caf_batch_request called with band[w][m] (band[m] when shared) and
 *   otherwise the same arguments; all five outputs follow that entry's parity statement.  Each (window, band, pair)
 *   chooses its own winner, the d-major first maximum with strict >, and dop_frac is the parabola through that slot's own
 *   three coarse peaks.
 * n_bands == 1 IS rmx_caf_batch_request with the same arguments (one checked request behind both): the same kernels, the
 *   same launches, bit-identical outputs.
 * Otherwise the forward kernels run unmasked -- plain, or under RMX_WEIGHT_PHAT whitened with the full band --, once per
 *   (window, buoy) un-rotated and once per (window, buoy, hypothesis) de-rotated, and the banded pair kernels
 *   (radio-mapper_amd/csrc/xspec_bands.hpp) mask the product, operand j from the de-rotated set.  A dropped bin is a stored
 *   +0 in the single-band search and a zeroed product here, and a kept bin is the product of the same two stored values:
 *   slot (w, m, q) carries the bits of the single-band call with band m.  The exception is rmx_xcorr_batch_bands': on the
 *   four-step route with the default pair list from 6 buoys on, the single-band call's peaks come from g_rows_anchor,
 *   which the banded call never takes; there the slot is held to the reference's bars.
 *   - N = 4096, every hypothesis in one launch (rmx_caf_batch's condition with n_dopplers * n_windows * n_bands virtual
 *     windows under 2^20; the spectra bound is unchanged): two forward launches, ONE banded pair launch over virtual
 *     windows v = (d * n_windows + w) * n_bands + m -- operand j at window v / n_bands of the de-rotated set, operand i,
 *     the band and the lag interval at virtual window v mod (n_windows * n_bands), the output slot v --, and the
 *     selection over [n_dopplers][n_windows * n_bands * n_pairs].
 *   - N = 4096 in chunks, the small route, the four-step route: per chunk one un-rotated forward pass, then per hypothesis
 *     one de-rotated forward pass, the banded pair kernels and k_caf_select(_fd) on the chunk's windows * n_bands *
 *     n_pairs slots.  The chunk is that of rmx_xcorr_batch_bands for n_bands bands.
 * Refusals (RMX_E_INVAL, the text in rmx_last_error, nothing staged or written), in this order: the search's head (a NULL
 *   buffer, band_cps included; a misaligned device pointer; n_dopplers); n_bands outside 1 .. 64; the batch shape and the
 *   pair list; the weighting and the bands, the text naming the window and the band index; the bounds; dop_frac
 *   overlapping another output -- every extent n_windows * n_bands * n_pairs elements; then the route: n_bands * n_pairs
 *   slots per window that no chunk of the ctx holds are refused with a text naming n_bands, never split silently.
 *   n_windows == 0 or n_pairs == 0 returns RMX_OK and writes nothing.
 * There is no integration here, and no refinement or quality: rmx_caf_batch_integrated and rmx_caf_batch_quality take one
 * band per window. */
int rmx_caf_batch_bands(rmx_ctx* ctx, const void* iq, int n_windows, const int32_t* pairs, int n_pairs,
                        const double* doppler_cps, int n_dopplers,
                        const double* band_cps, int n_bands, int bands_per_window, unsigned weighting,
                        const int32_t* lag_bounds, int bounds_per_window,
                        int32_t* dop_idx, float* dop_frac,
                        int32_t* lag_int, float* lag_frac, float* peak, unsigned flags);

/* Batched hyperbolic position solve: the consumer of the lags.  One
 * independent 3-unknown least-squares problem per window with the reference's objective
 * (HyperbolicPositioning.triangulate_position, tdoa_processor.py:249-273),
 *     f(p) = sum_q weight[w][q] * ( |p - b_j| - |p - b_i| - d[w][q] )^2 ,  (i, j) = pairs[q],
 *     d = (lag_int + lag_frac) / sample_rate_hz * 299792458  (tdoa_processor.py:141,169-170),
 * started from the centroid of the buoys (tdoa_processor.py:275-280).  The reference minimises f
 * with scipy BFGS one window at a time; this entry uses a fixed Levenberg-Marquardt rule in float64
 * (lambda_0 = 1e-3 on diag(J^T J); accept on decrease: lambda /= 3, floor 1e-12; reject: lambda *= 4;
 * stop at an accepted step < 1e-4 m, lambda > 1e12, or max_iter iterations), restated on the CPU in
 * oracle/solve_ref.py.
 *   buoy_xyz   host double [n_buoys][3], ECEF metres (GeodeticCalculator.lat_lng_to_xyz)
 *   pairs      host int32 [n_pairs][2] or NULL for all i<j in nested-loop order
 *   lag_int / lag_frac   [n_windows][n_pairs], exactly what rmx_xcorr_batch wrote (device pointers
 *              with RMX_IN_DEVICE: the two calls chain on the ctx stream without a host round trip)
 *   weight     float [n_windows][n_pairs] = 1/(confidence+0.1) (tdoa_processor.py:267), or NULL = 1
 *   pos        double [n_windows][3]  ECEF metres        cost    double [n_windows]  f at pos
 *   iters      int32  [n_windows]     iterations used    (device pointers with RMX_OUT_DEVICE)
 * accuracy_meters of the reference = sqrt(cost / n_pairs) (tdoa_processor.py:300).
 * Parity: pos, cost and iters are bit-identical, for every window, to tests/solve_kernel_ref.py, the float64 restatement
 *   of k_solve that keeps the kernel's order of sums and products with one rounding per operation (no contraction into
 *   fma; f64 divide and square root are correctly rounded).  The pair list is used as given: repeats, reversed pairs
 *   and (i, i) are legal; swapping every pair to (j, i) while negating lag_int and lag_frac gives the same bits.
 *   weight == NULL gives the bits of a weight array of ones.  oracle/solve_ref.py states the same rule with other sums
 *   (numpy @, LU) and agrees to 1e-6 relative in the cost on the windows that reach the global minimum.
 * Degenerate input gives finite outputs and the documented give-up: where no step can be accepted (all weights zero; the
 *   centroid exactly on a buoy, which makes every Jacobian entry NaN; a failed Cholesky every time) the 25th rejection
 *   takes lambda from 1e-3 past 1e12, so iters = min(25, max_iter), pos = the start point (the centroid) and cost = f
 *   there.  A NaN trial cost compares false and counts as a rejection.
 * Refusals (RMX_E_INVAL, rmx_last_error set, no output written): a NULL buffer, n_buoys outside 2..64, sample_rate_hz not
 *   positive (NaN included), max_iter < 1, n_windows < 0, pairs == NULL with n_pairs neither 0 nor n_buoys (n_buoys - 1) / 2,
 *   a custom list of fewer than 1 or more than 2016 pairs, a pair index outside 0..n_buoys-1.  n_windows == 0 returns
 *   RMX_OK and writes nothing. */
int rmx_solve_batch(rmx_ctx* ctx, const double* buoy_xyz, int n_buoys, const int32_t* pairs, int n_pairs,
                    const int32_t* lag_int, const float* lag_frac, const float* weight,
                    double sample_rate_hz, int n_windows, int max_iter, double* pos, double* cost,
                    int32_t* iters, unsigned flags);

/* rmx_solve_batch with a surface constraint and with the figures that say how far the fix can be trusted: the
 * information matrix at the fix, its inverse and the residual of every pair.  Every argument of rmx_solve_batch means
 * what it means there; RMX_IN_DEVICE and RMX_OUT_DEVICE act as there, and info, cov and resid follow RMX_OUT_DEVICE with
 * pos, cost and iters, so the call chains on the ctx stream.
 *   plane      host double [9] = origin o, then two orthonormal directions e1, e2, all ECEF (for stations on the sea:
 *              GeodeticCalculator.tangent_plane at the fleet's centroid), or NULL = three unknowns.
 *   plane == NULL: pos, cost and iters are those of rmx_solve_batch with the same arguments bit for bit (the same kernel).
 *   plane given: two unknowns u = (u1, u2), p(u) = o + u1 e1 + u2 e2.  The objective f is rmx_solve_batch's; the start is
 *              the centroid of the buoys projected onto the plane; the Jacobian row of a pair is (j . e1, j . e2) with the
 *              j of the three-unknown solve; the Levenberg-Marquardt rule is rmx_solve_batch's written out for 2 x 2
 *              (lambda_0 = 1e-3 on diag(J^T W J); a Cholesky step; a failed factorisation or a NaN trial cost is a
 *              rejection; accept: lambda /= 3, floor 1e-12; reject: lambda *= 4; stop at an accepted step < 1e-4 m,
 *              lambda > 1e12, or max_iter).  pos = p(u) in ECEF, cost = f there.
 * At the returned pos, in both modes:
 *   info       double, the undamped J^T W J.  plane == NULL: [n_windows][6] = xx xy xz yy yz zz in ECEF; plane given:
 *              [n_windows][3] = 11 12 22 in plane coordinates.  In m^-2 where weight is in m^-2.
 *   cov        double, its inverse through Cholesky, in the same layout.
 *   resid      double [n_windows][n_pairs] = |p - b_j| - |p - b_i| - d in metres, or NULL: not computed.
 * Singular rule: the information is singular when a Cholesky pivot is <= 1e-12 * its own diagonal entry of info, or is
 *   not finite.  Then cov is +inf on its diagonal and 0 off it.  1e-12 sits four decades above float64 rounding and six
 *   below the weakest geometry that still carries information (five sea-level stations about 10 km apart solved for
 *   three unknowns: the last pivot is a few 1e-7 of its diagonal entry at the emitter, not singular; three such stations:
 *   1e-16 or an exact 0, singular).  If any entry of info
 *   is not finite (pos exactly on a buoy, which the give-up of rmx_solve_batch with the centroid on a buoy returns),
 *   info is written as zeros and cov as singular.  No output is ever NaN.
 * What the outputs mean:
 *   with weight = 1 / sigma_d^2 (sigma_d = the standard deviation of a pair's range difference in metres,
 *   xcorr.lag_weight) cov is the covariance of the fix under INDEPENDENT pair errors, and cost is a chi-square with
 *   (pairs of weight > 0) - (2 or 3) degrees of freedom;
 *   with weight == NULL cov is the cofactor matrix: the dilution of precision, squared.
 *   All pairs of B stations carry only B - 1 independent lags: their errors share receivers, they are NOT independent,
 *   and cov is then optimistic.  The entry does not correct for that.
 * Parity: every output is bit-identical to tests/solve_fix_ref.py, the kernel-order float64 restatement.
 * Refusals (RMX_E_INVAL, rmx_last_error set, no output written, the ctx stays usable): every refusal of rmx_solve_batch;
 *   info or cov NULL; a plane entry that is not finite; | |e1| - 1 | or | |e2| - 1 | above 1e-9; |e1 . e2| above 1e-9.
 *   n_windows == 0 returns RMX_OK and writes nothing. */
int rmx_solve_batch_fix(rmx_ctx* ctx, const double* buoy_xyz, int n_buoys, const int32_t* pairs, int n_pairs,
                        const int32_t* lag_int, const float* lag_frac, const float* weight,
                        double sample_rate_hz, const double* plane, int n_windows, int max_iter, double* pos,
                        double* cost, int32_t* iters, double* info, double* cov, double* resid, unsigned flags);

/* Spectral detection: the reference's per-capture detector
 * (buoy_node.py:401-433, iq_stream_client.py:186-217) batched over windows.  Per window of n_samples
 * (power of two, 16..16384; independent of the ctx's n_samples) complex samples:
 *     P[k] = 20 log10(|FFT_N(iq)[k]| + 1e-12)                            (float32, unpadded, unwindowed)
 *     peaks = scipy.signal.find_peaks(P, height=threshold_db, distance=distance)   (buoy_node.py:411-415)
 *             (local maxima, a plateau at its midpoint (the lower middle bin), none at bin 0 or n_samples-1; kept
 *             when P >= (float)threshold_db; then highest-first removal of every peak closer than distance bins to
 *             a kept one.  Exact ties in P rank the higher bin first: scipy's own order on exact ties comes from
 *             numpy's unstable argsort and is unspecified.  Any distance >= n_samples acts as n_samples: only the
 *             highest candidate is kept.)
 *     floor = median(P); snr = P[peak] - floor; confidence = min(max(snr/20, 0), 1) (buoy_node.py:425-427)
 *     a peak is reported unless |signed FFT bin| < dc_exclude_bins (the +-10 kHz of buoy_node.py:419,
 *     i.e. 10e3 * n_samples / sample_rate) or confidence < min_confidence (0.3, buoy_node.py:430)
 *   iq          complex64 [n_windows][n_samples] (or uint8 I,Q pairs with RMX_IN_U8); device with RMX_IN_DEVICE
 *   count       int32 [n_windows]   peaks found (may exceed max_peaks; the arrays hold the first max_peaks,
 *               in ascending bin order as find_peaks returns them; entries past min(count, max_peaks) are undefined)
 *   bin / power_db / snr_db / confidence   [n_windows][max_peaks];  noise_floor_db float [n_windows]
 *   (device pointers with RMX_OUT_DEVICE).  Frequency of a bin: fftfreq, f_centre + (bin < N/2 ? bin : bin - N) * fs / N. */
int rmx_detect_batch(rmx_ctx* ctx, const void* iq, int n_windows, int n_samples, float threshold_db, int distance,
                     double dc_exclude_bins, float min_confidence, int max_peaks, int32_t* count, int32_t* bin,
                     float* power_db, float* snr_db, float* confidence, float* noise_floor_db, unsigned flags);

/* Wait for all work queued on the ctx stream. */
int rmx_synchronize(rmx_ctx* ctx);

/* With option "timing"=1: accumulated HIP-event times of the last rmx_xcorr_batch call, per kernel
 * family (forward-spectrum kernels, pair kernels), and the number of launches of each.  Waits for
 * the stream.  Any pointer may be NULL. */
int rmx_last_timing(rmx_ctx* ctx, float* fwd_ms, int* fwd_launches, float* pair_ms,
                    int* pair_launches);

/* The same per kernel family of EVERY path (N = 4096, whole-window, four-step, CAF): kind = 0, 1, 2, ... until the call
 * returns RMX_E_INVAL; *name is a static string ("k_win|k_pair", "g_cols_fwd", "g_rows_fused", "g_rows_anchor",
 * "g_cols_inv", "g_final", "g_win_*", ...), *ms the summed HIP-event time of that family's launches in the last
 * rmx_xcorr_batch / rmx_caf_batch call, *launches their number.  Diagnostic only: no reference counterpart (the
 * reference times nothing on this path); bench.py reports it per BASELINE shape.  Any pointer may be NULL. */
int rmx_last_timing_kind(rmx_ctx* ctx, int kind, const char** name, float* ms, int* launches);

/* Static text naming what this binary was built from: "RMX_BUILD_INFO source_digest=<16 hex> arch=gfx950", the digest
 * being sha256 over the kernel sources, this header and the compiler flags as __graft_entry__.source_digest() computes
 * it.  bench.py prints it beside the digest of the sources it sees and refuses to run on a mismatch; never fails. */
const char* rmx_build_info(void);

/* Bytes of device scratch the ctx holds (spectra, tables, staging). */
size_t rmx_scratch_bytes(const rmx_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* RMX_H */
