/* libmcorr -- MI355X (gfx950) motion-correction kernels, C ABI.
 *
 * Drop-in boundary for the estimate -> correct hot path of
 * teamtomo/torch-motion-correction.  The reference has no FFI of its own (it is pure
 * Python on torch ops), so these entry points are what a
 * binding of that path needs: plain device pointers, sizes and a hipStream_t passed
 * as void*.  No torch types appear here.  Every function is asynchronous on
 * `stream`, allocates nothing, never synchronises, and returns 0 (MC_OK), a negative
 * MC_ERR_* code, or a positive hipError_t from the launch.
 *
 * All pointers are DEVICE pointers unless marked (host).  Complex values are
 * interleaved float pairs (re, im).  The Python host layer that mirrors the
 * reference's function signatures on top of this ABI is
 * torch_motion_correction_amd/ (ctypes); INTEGRATION.md shows the binding.
 *
 * Reference citations are relative to /root/reference/src/torch_motion_correction/.
 */
#ifndef MCORR_H
#define MCORR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCORR_ABI_VERSION 1
int mc_abi_version(void);

/* Geometry of one pruned 2-D real transform (host struct, passed by pointer).
 * W,H: transform size (powers of two: 32<=W<=8192, 16<=H<=4096).
 * nkx: kept rfft columns [0,nkx).  kyp,kyn: kept ky rows [0,kyp) U [H-kyn,H).
 * [y0,y0+ny) x [x0,x1): window region that can be non-zero (support of the mask);
 * ny and H must be multiples of RG (rows per workgroup, 1..16); x0,x1 even. */
typedef struct mc_xc_geom {
  int W, H, nkx, kyp, kyn, y0, ny, x0, x1, RG;
} mc_xc_geom;

/* ---- plan constants ------------------------------------------------------------ */

/* Soft-edged disk mask (h*w floats): replaces torch_grid_utils.circle as called at
 * estimate_motion_xc.py:69-74 and :262-264 -- 1 where |p-c| < radius (c = (h//2,w//2)),
 * cos(pi/2 * d/smoothing_radius) of the exact Euclidean distance transform d to the
 * disk for 0 < d <= smoothing_radius, else 0.  A radius that no pixel is inside of
 * (radius = 0: the test is strict, the centre pixel has distance 0) leaves no disk to
 * measure a distance to: the table is all zeros, whatever the smoothing radius.
 * halfw: scratch of h ints. */
int mc_circle_mask(float* mask, int* halfw, int h, int w, float radius, float smoothing_radius,
                   void* stream);

/* Combined band-pass * B-factor envelope on the pruned grid, filt[kx][kyi]
 * (nkx * (kyp+kyn) floats): replaces b_envelope (estimate_motion_xc.py:81-88,:266-273)
 * and prepare_bandpass_filter/bandpass_filter (utils.py:87-114) -- value
 * exp(-B*(f/pixel_size)^2/4) where low < f <= high (cycles/px), else 0. */
int mc_xc_filter(float* filt, const mc_xc_geom* geom, float low, float high, float b_factor,
                 float pixel_size, void* stream);

/* storage types of frame data (the values of mc_condition_movie's `kind`) */
#define MC_STORE_U8 0
#define MC_STORE_I16 1
#define MC_STORE_F16 2
#define MC_STORE_F32 3

/* ---- a2: normalize_image statistics (utils.py:49-84) ---------------------------- */
/* mean and unbiased std of stack[:, hl:hu, wl:wu] over all t frames jointly, the frames in their storage
 * type (MC_STORE_F32 / MC_STORE_F16: statistics of the fp32 up-cast, read straight from the fp16 bytes).
 * acc: 2 doubles of scratch; out3 = {mean, 1/std, std} as floats. */
int mc_central_box_stats_t(const void* stack, int storage, int t, int h, int w, int hl, int hu, int wl,
                           int wu, double* acc, float* out3, void* stream);
/* dst = (src - mean) * (1/std), n elements (normalize_image's elementwise pass). */
int mc_normalize(const float* src, float* dst, int64_t n, const float* mean_rstd, void* stream);

/* ---- a1/a6/a8: cross-correlation shift search ----------------------------------- */
/* Dynamic LDS bytes K1/K4 need for this geometry (host helper). */
int mc_xc_rows_lds_bytes(const mc_xc_geom* geom);

/* K1.  For each job j: window origin src + job_off[j], rows row_stride floats apart;
 * each sample becomes (x-mean)*rstd*mask^expo[j] (mask: H*W floats or NULL;
 * mean_rstd NULL = no normalisation; job_expo NULL = exponent 1); real FFT along x;
 * first nkx bins -> T1[j][kx][ny] (complex).  estimate_motion_xc.py:66,77-78 / :339-345. */
int mc_xc_rows_forward(const float* src, const int64_t* job_off, int64_t row_stride,
                       const int* job_expo, const float* mask, const float* mean_rstd, void* T1,
                       const void* tw_row, int njobs, const mc_xc_geom* geom, void* stream);

/* N2, fused conditioning (examples/ttMotion.py:90-121 gain_correct, :180-199 set_frames_mean_zero, done on
 * the fly by the kernels that read the raw bytes: no conditioned fp32 movie exists).  One pass over a raw
 * (t,h,w) movie of storage `kind` (MC_STORE_*) and its optional (h,w) gain reference:
 *   stats[3 f ..] = { sum v, sum_box v, sum_box v^2 },  v = raw * gain,  box = [hl,hu) x [wl,wu) -- the central box of
 *   normalize_image (utils.py:76-81);   mu[f] = mean of frame f (0 when mean_zero == 0);
 *   mean_rstd = {mean, 1/std} of the conditioned box values of ALL frames jointly (unbiased, utils.py:82-83);
 *   sub[f] = mu[f] + mean: what mc_xc_rows_forward_raw subtracts from raw * gain. */
int mc_raw_movie_stats(const void* raw, int kind, const float* gain, int nframes, int h, int w, int hl, int hu,
                       int wl, int wu, int mean_zero, double* stats, float* mu, float* sub, float* mean_rstd,
                       void* stream);

/* N2 with the hot-pixel step (examples/ttMotion.py:127-172; rule of mc_condition_movie_hot), still without a
 * conditioned fp32 movie.  The raw K1 and the raw warp run on the unreplaced samples v = raw * gain; each hot
 * pixel is then applied as a sparse correction by delta = r - v (r: its replacement), both consumers being
 * linear in the sample.  Sequence per movie:
 *  1. mc_raw_hot_detect: one pass for stats (as mc_raw_movie_stats, before replacement) and hstats[f][3] =
 *     {sum v, sum v^2, -} of the whole frame, then the detection pass: every hot pixel takes a slot of the list
 *     keys[i] = f*h*w + pixel index, rv[2i..] = {r, v}; *counter = number of hot pixels (may exceed `capacity`:
 *     then only `capacity` entries were written and the list is unusable), counts[f] = per frame.  gain is
 *     required (pass ones for none); w % 8 == 0 and 8-byte (u8) / 16-byte aligned raw, 16-byte aligned gain,
 *     else MC_ERR_UNSUPPORTED.
 *  2. the caller sorts the n = *counter entries by key (ascending) -- the fixed order every later step sums in.
 *  3. mc_raw_hot_finalize: stats corrected for the replacement, then mu / sub / mean_rstd as
 *     mc_raw_movie_stats gives them, for the frames AFTER replacement (mu rounded as mc_condition_movie_hot).
 *  4. mc_xc_rows_hot_correct after K1 (mc_xc_rows_forward_raw / mc_xcg_rows_forward_raw) of frames
 *     [frame0, frame0 + njobs): adds (r - v) * rstd * mask(y,x) * exp(-2 pi i kx x / W) to T1[f - frame0][kx][y - y0]
 *     for every kept bin; one workgroup per (frame, row), no atomics.
 *  5. after mc_warp_rigid_raw (its weight tables in `scratch`): mc_warp_rigid_hot_taps writes n * 49 records
 *     (key = f*h*w + output pixel or INT64_MAX, value = (r - v) * the warp's weight of q for that output);
 *     the caller sorts them stably by key (for the sum: by key mod h*w) and mc_hot_scatter_add adds every
 *     run of equal keys < limit, summed in order, to out[key] (the frames, or the sum with limit = h*w). */
int mc_raw_hot_detect(const void* raw, int kind, const float* gain, int nframes, int h, int w, int hl, int hu,
                      int wl, int wu, float threshold, double* stats, double* hstats, long long* keys, float* rv,
                      long long capacity, unsigned long long* counter, int* counts, void* stream);
int mc_raw_hot_finalize(const long long* keys, const float* rv, int64_t n, int nframes, int h, int w, int hl, int hu,
                        int wl, int wu, int mean_zero, const double* hstats, double* stats, float* mu, float* sub,
                        float* mean_rstd, void* stream);
int mc_xc_rows_hot_correct(const long long* keys, const float* rv, int64_t n, int frame0, int njobs, int h, int w,
                           const float* mask, const float* mean_rstd, void* T1, const mc_xc_geom* geom, void* stream);
int mc_warp_rigid_hot_taps(const long long* keys, const float* rv, int64_t n, int nframes, int h, int w,
                           const float* scratch, long long* rec_key, float* rec_val, void* stream);
int mc_hot_scatter_add(const long long* key, const float* val, int64_t m, int64_t limit, float* out, void* stream);

/* Input conditioning of raw detector frames (caller-side steps of the reference's pipeline,
 * examples/ttMotion.py:90-121 gain multiply and :174-199 per-frame mean-zero):
 * out[f] = raw[f] * gain - mean(raw[f] * gain), fp32 out.  kind: storage type of raw, 0 = u8,
 * 1 = i16, 2 = f16, 3 = f32; gain: (h*w) floats or NULL; mean_zero != 0 needs `sums`
 * (nframes doubles of scratch).  hw = pixels per frame. */
int mc_condition_movie(const void* raw, int kind, const float* gain, int nframes, int64_t hw,
                       int mean_zero, double* sums, float* out, void* stream);
/* The same with the example pipeline's hot-pixel step between the gain multiply and the mean-zero
 * step (examples/ttMotion.py:127-172): a pixel of v = raw * gain is hot when it lies more than
 * `threshold` population standard deviations from its frame's mean -- the example's detection,
 * reproduced exactly.  Replacement: the example draws a RANDOM neighbour; here (documented as
 * ours) the mean of the up-to-8 neighbours that are not hot themselves, from the frame before any
 * replacement (the frame mean if all are hot).  The mean subtracted afterwards is the mean AFTER
 * replacement.  stats: 3 * nframes doubles of scratch (sum, sum of squares, replacement delta);
 * hot_count: nframes ints (number of hot pixels per frame) or NULL. */
int mc_condition_movie_hot(const void* raw, int kind, const float* gain, int nframes, int h, int w,
                           int mean_zero, float threshold, double* stats, int* hot_count, float* out,
                           void* stream);

/* Dose-weighted accumulation in Fourier space (the caller-side exposure filter of the
 * reference's pipeline, examples/ttMotion.py:331-351, crit_exposure_bfactor = -1):
 * A[kx][ky] (+)= sum_j q_{frame0+j}(k) * S[j][kx][ky] over the nframes full spectra in S
 * ([j][W/2+1][H] complex, as K1+K2 with the full geometry produce them); first != 0 starts A
 * from zero, last != 0 applies 1/sqrt(sum over all total_frames of q^2).  An inverse
 * transform of A (mc_fourier_shift_cols_inverse with zero shifts + mc_xc_rows_inverse_store)
 * then gives sum_f irfft2(q_f * rfft2(frame_f)).  q_f = exp(-0.5 N_f / N_c(k)), Grant &
 * Grigorieff 2015; third-party semantics, parity unpinned (oracle/thirdparty_semantics.py). */
int mc_dose_accumulate(const void* S, int nframes, int frame0, int total_frames, void* A, int W,
                       int H, float pixel_size, float pre_exposure, float dose_per_frame,
                       float voltage, int first, int last, void* stream);

/* K1 for rows of 1024 samples (1024 x 1024 patches; needs W == 1024, nkx <= 128, ny % 8 == 0,
 * a mask, every exponent >= 1; MC_ERR_UNSUPPORTED otherwise): one wavefront per row, and with
 * expo_b != NULL the same samples are transformed twice, with mask^expo_a[j] into T1a and
 * mask^expo_b[j] into T1b -- the U and V spectra of the mean-except-current reference
 * (estimate_motion_xc.py:315-346) from one read of the patch rows.  Layouts as
 * mc_xc_rows_forward; row_chord: NULL or as in mc_xc_rows_forward_stats_t.  The samples are read in their
 * storage type (MC_STORE_F32 or MC_STORE_F16; job_off and row_stride in elements): an fp16 movie is
 * transformed without an fp32 copy of it.  Results are those of the fp32 up-cast (the reference cannot run
 * Half on the CPU at all). */
int mc_xc_rows_forward_dual_t(const void* src, int storage, const int64_t* job_off, int64_t row_stride,
                              const int* expo_a, const int* expo_b, const float* mask,
                              const float* mean_rstd, void* T1a, void* T1b, const void* tw_row,
                              int njobs, const mc_xc_geom* geom, const int* row_chord, void* stream);

/* Column-transform engine of K2 / the near-window K3: 0 = automatic (H == 4096 with at most
 * 512 kept rows at either end of the spectrum -> register-resident radix-16 transform;
 * H == 1024 with at most 128 -> one wavefront per column, mc_wave_fft.h),
 * 1 = always the radix-8 Stockham passes.  Process-wide; results agree to fp32 rounding. */
int mc_xc_col_engine(int mode);

/* Row-transform engine of K1: 0 = automatic (W == 4096, nkx <= 512, no per-job exponents,
 * 16-byte aligned src/mask and row_stride % 4 == 0 -> one wavefront per row, mc_wave_fft.h;
 * job_off[] must then be multiples of 4 floats, as whole-frame offsets f*h*w are),
 * 1 = always one workgroup per row.  Process-wide; results agree to fp32 rounding. */
int mc_xc_row_engine(int mode);

/* m0 = {mean of the n samples at x (MC_STORE_F32 / MC_STORE_F16), 1, 1}: the provisional mean
 * mc_xc_rows_forward_stats_t takes (one small workgroup; any value near the true mean serves). */
int mc_xc_provisional_mean_t(const void* x, int storage, int n, float* m0, void* stream);

/* K1 with the normalisation statistics fused in (whole-frame jobs only): samples become
 * (x - m0[0]) * mask (m0: device float[3] = {provisional mean, 1, 1}); while reading, the
 * sums of (x-m0) and (x-m0)^2 over the central box rows [hl,hu) x cols [wl,wu) (window
 * coordinates, inside the mask support, wl/wu even) of every job are accumulated;
 * afterwards fix = {mean - m0, 1/std} and out3 = {mean, 1/std, std} (unbiased std over
 * all jobs jointly, utils.py:76-84).  acc: 128 doubles scratch (64 x {sum, sumsq}).  Feed `fix` to
 * mc_xc_cols_forward_fix, which finishes the normalisation by linearity.
 * row_chord (NULL, or H x 2 ints per WINDOW row y: first and last 4-aligned column whose quad
 * holds a non-zero mask value): samples outside a row's chord of the mask disk are not fetched
 * (they are multiplied by the mask's exact zero) -- 21 % of the support box of a circular mask.
 * The statistics box must lie inside the chords (the caller checks; plan.row_chords).
 * The frames are read in their storage type (MC_STORE_F32 / MC_STORE_F16; job_off and row_stride in
 * samples): fp16 frames are read as they are by the wavefront-per-row kernel (4096-column frames;
 * MC_ERR_UNSUPPORTED otherwise: widen the stack and call again with MC_STORE_F32). */
int mc_xc_rows_forward_stats_t(const void* src, int storage, const int64_t* job_off, int64_t row_stride,
                               const float* mask, const float* m0, void* T1, const void* tw_row,
                               int njobs, const mc_xc_geom* q, int hl, int hu, int wl, int wu,
                               double* acc, float* fix, float* out3, const int* row_chord, void* stream);

/* N2: K1 from the raw bytes of a u8 / i16 movie, conditioned on the fly (no fp32 movie):
 *   rows of (raw * gain - job_sub[job]) * mean_rstd[1] * mask  ->  T1, as mc_xc_rows_forward writes it.
 * `gain` has the frames' row pitch (whole-frame jobs); job_sub / mean_rstd come from mc_raw_movie_stats;
 * follow with mc_xc_cols_forward / mc_xcg_cols_forward (no fix-up: the statistics are known before this pass).
 * mc_xc_rows_forward_raw: power-of-two widths (4096 columns with 16-byte aligned buffers and row_stride % 8 == 0 on
 * the wave-per-row engine, the others on the workgroup engine); mc_xcg_rows_forward_raw: rows of 5760 / 11520
 * samples (the K3 formats; `line` = the direct 2880 / 5760-point plan).  Anything else: MC_ERR_UNSUPPORTED. */
int mc_xc_rows_forward_raw(const void* raw, int storage, const float* gain, const int64_t* job_off,
                           int64_t row_stride, const float* mask, const float* job_sub, const float* mean_rstd,
                           void* T1, const void* tw_row, int njobs, const mc_xc_geom* q, const int* row_chord,
                           void* stream);

/* N2: the patch estimator's 1024-sample rows (mc_xc_rows_forward_dual_t's wave-per-row engine) from the raw bytes
 * of a u8 / i16 movie: rows of (raw * gain - job_sub[job]) * mean_rstd[1] * mask^expo_a (and mask^expo_b into T1b
 * when expo_b is given) -> T1a / T1b.  Patch jobs: job_off / row_stride in samples of the movie; the gain has the
 * frames' row pitch and a job's gain values sit at job_off[job] % frame_area (its offset within its frame);
 * job_sub[job] = the job's frame mean + the box mean (mc_raw_movie_stats).  Geometries the wave engine does not
 * take (W != 1024, nkx > 128, ny % 8) and other storage tags: MC_ERR_UNSUPPORTED. */
int mc_xc_rows_forward_dual_raw(const void* raw, int storage, const float* gain, int64_t frame_area,
                                const int64_t* job_off, int64_t row_stride, const int* expo_a, const int* expo_b,
                                const float* mask, const float* job_sub, const float* mean_rstd, void* T1a, void* T1b,
                                const void* tw_row, int njobs, const mc_xc_geom* q, const int* row_chord,
                                void* stream);

/* K2.  Column FFT of T1, kept ky rows, times filt (or NULL) -> S[j][kx][kyi].
 * estimate_motion_xc.py:78,98 / :340-346. */
int mc_xc_cols_forward(const void* T1, const float* filt, void* S, const void* tw_col, int njobs,
                       const mc_xc_geom* geom, void* stream);
/* K2 with the linear normalisation fix-up: S = filt * fix[1] * (Y - fix[0] * Mhat), Mhat =
 * pruned spectrum of the mask ([kx][kyi] complex, i.e. K1+K2 of an all-ones window). */
int mc_xc_cols_forward_fix(const void* T1, const float* filt, void* S, const void* tw_col,
                           int njobs, const mc_xc_geom* geom, const float* fix, const void* Mhat,
                           void* stream);

/* K3.  pair p: conj(S_ref[ref_idx[p]]) * S_cur[cur_idx[p]] * scale, inverse column FFT
 * -> T2[p][kx][H].  estimate_motion_xc.py:112-113 / :349-350. */
int mc_xc_cols_inverse(const void* S_cur, const int* cur_idx, const void* S_ref,
                       const int* ref_idx, void* T2, const void* tw_col, float scale, int npairs,
                       const mc_xc_geom* geom, void* stream);

/* Rows stored per end of the map by the near-window search below (searched rows + guard rows). */
int mc_xc_near_rows(const mc_xc_geom* geom);

/* K3+K4+K5 for the arg-max search without materialising the map or T2 (power-of-two
 * W and H >= 256; estimate_motion_xc.py:106-123).  Rows [0, n) and [H-n, H) of the
 * correlation map (n = mc_xc_near_rows(geom)) are transformed from T2_near
 * ([p][kx][2n] complex) while the column pass accumulates the per-row triangle-inequality
 * bounds of ALL rows; only if a far row's bound can still reach the near-window maximum are
 * the full column pass (T2_full, [p][kx][H]) and the far row groups evaluated, a decision
 * taken on the device (the fallback kernels are enqueued and return at once).  The result
 * is the exact arg-max of the full map either way.  n counts the searched rows plus a few
 * guard rows, so that nb (optional, [p][3][3] floats: the map around every peak as
 * mc_xc_peak_neighbourhood gives it, for the sub-pixel parabola fit of
 * estimate_motion_xc.py:414-483) can be taken from T2_near too.  part_val: npairs*(H/RG) +
 * npairs*H floats; part_idx: npairs*(H/RG) + npairs + 1 ints.
 * shift_rows (optional): pair p's shift goes to row shift_rows[p] of a (n_shift_rows, 2) table
 * that is zeroed first (rows no pair writes -- the reference frame -- stay exactly zero,
 * estimate_motion_xc.py:102); NULL: shifts is (npairs, 2), row p. */
int mc_xc_correlate_argmax(const void* S_cur, const int* cur_idx, const void* S_ref,
                           const int* ref_idx, void* T2_full, void* T2_near, float* part_val,
                           int* part_idx, int* peaks, float* shifts, const int* shift_rows,
                           int n_shift_rows, float* nb, const void* tw_col, const void* tw_row,
                           float scale, int npairs, const mc_xc_geom* geom, void* stream);

/* K4+K5.  Inverse real row FFT of T2 fused with the arg-max (first maximum, as
 * torch.argmax): peaks[p] = flat index y*W+x, shifts[p] = (sy,sx) after the
 * wrap-around rule `p if p <= n//2 else p-n`.  part_val: scratch of npairs*(H/RG) +
 * npairs*H floats; part_idx: scratch of npairs*(H/RG) + npairs ints.  The search is an exact
 * branch and bound: row groups whose triangle-inequality bound cannot reach the best
 * value found so far are skipped.  estimate_motion_xc.py:113-121 / :350-355,368-369. */
int mc_xc_rows_inverse_argmax(const void* T2, float* part_val, int* part_idx, int* peaks,
                              float* shifts, const void* tw_row, int npairs,
                              const mc_xc_geom* geom, void* stream);

/* K6.  nb[p][3][3]: correlation values at (py-1..py+1, px-1..px+1) around peaks[p]
 * (NaN outside the map), same arithmetic as K4.  Feeds the parabola fit of
 * _apply_sub_pixel_refinement, estimate_motion_xc.py:414-483. */
int mc_xc_peak_neighbourhood(const void* T2, const int* peaks, float* nb, const void* tw_row,
                             int npairs, const mc_xc_geom* geom, void* stream);

/* Reference spectra for reference_strategy="mean_except_current"
 * (estimate_motion_xc.py:310-328 + the in-place mask aliasing):
 * REF[f][g] = inv_count * sum_{o != f} (o in S_f ? V[o][g] : U[o][g]), spectra of `len`
 * complex values, g in [0,npatch).  The sets S_f come as a schedule the
 * host derives from the memo replay: frame f either adds sched_idx[sched_ptr[f] ..
 * sched_ptr[f+1]) to the running set (sched_rebuild[f] == 0) or replaces the set by that
 * list (sched_rebuild[f] == 1). */
int mc_xc_ref_mean_except_current(const void* U, const void* V, const int* sched_ptr,
                                  const int* sched_idx, const uint8_t* sched_rebuild, void* REF,
                                  int t, int npatch, int64_t len, float inv_count, void* stream);

/* Iterative sub-pixel whole-frame alignment (refine_global_motion; no counterpart in the reference tree, whose
 * example calls a refine_alignment it never shipped, examples/ttMotion.py:264-285).  One iteration on the filtered
 * spectra S ([t][nkx][nky] complex, as K2 writes them) with the current shifts_px ([t][2] px, (y, x)):
 *   G_f = S_f exp(+2 pi i (fy[ky] sy_f + fx[kx] sx_f))   (fy, fx: the kept bins' signed frequencies in cycles/px, the
 *   convention of mc_local_loss_sums; the ramp correct_motion_fast applies for the field s),
 *   A = sum_f G_f,   REF[f] = (A - G_f) / (t - 1)   (zero for t == 1),
 *   G[f] = G_f exp(-2 pi i under_px (fy + fx)): the aligned frame UNDER-corrected by under_px pixels on both axes, so
 *   that the correlation map of (cur = G, ref = REF) is the true one translated circularly by (under_px, under_px)
 *   and a converged peak lies inside the map, where mc_xc_peak_neighbourhood has values (0: G = G_f).
 * 1 <= t <= 512.  Follow with K3/K4/K6 on (G, REF) and mc_xc_refine_update. */
int mc_xc_aligned_refs(const void* S, const float* shifts_px, const float* fy, const float* fx, void* G, void* REF,
                       int t, int nkx, int nky, int under_px, void* stream);
/* The rest of the iteration, one small workgroup: for every frame f the residual r_f = (peak - under_px) mod (H, W)
 * after the wrap-around rule `p if p <= n//2 else p-n`, plus the parabola offsets of estimate_motion_xc.py:465-481
 * from nb ([t][3][3], its `!=` guards; an axis whose outer samples are NaN -- a peak on the border of the translated
 * map -- keeps its integer residual); shifts_px[f] += (t-1)/t r_f, then shifts_px -= shifts_px[ref] with row `ref`
 * exactly 0; *max_r = max_f max(|r_y|, |r_x|).  2 <= t <= 512. */
int mc_xc_refine_update(const int* peaks, const float* nb, float* shifts_px, int ref, int t, int H, int W,
                        int under_px, float* max_r, void* stream);

/* Iterative sub-pixel PATCH alignment (refine_local_motion): the same iteration with one shift per (frame, patch).
 * S: the patch estimator's filtered spectra, [t][npatch][nkx][nky] complex (job = f * npatch + q); shifts_px and
 * offsets_px: [t][npatch][2] px (y, x), offsets_px the whole-pixel displacement each job's window was cut at (the
 * ramp carries shifts_px - offsets_px).  For the patches q0 <= q < q0 + nq (independent of each other):
 *   G_fq = S_fq exp(+2 pi i (fy[ky] (sy - oy) + fx[kx] (sx - ox))),   REF = (sum_g G_gq - G_fq) / (t - 1),
 * G (under-corrected by under_px on both axes, as mc_xc_aligned_refs) and REF hold that range only, [t][nq][nkx][nky]:
 * pair f * nq + (q - q0) for K3/K4/K6.  1 <= t <= 512, nq <= 65535. */
int mc_xc_aligned_refs_patches(const void* S, const float* shifts_px, const float* offsets_px, const float* fy,
                               const float* fx, void* G, void* REF, int t, int npatch, int q0, int nq, int nkx,
                               int nky, int under_px, void* stream);
/* mc_xc_refine_update for the patches q0 <= q < q0 + nq, one workgroup each: peaks / nb in the pair order above;
 * shifts_px[f][q] += (t-1)/t r, then shifts_px[:][q] -= shifts_px[ref][q] (row `ref` exactly 0 in every patch);
 * max_r[q] ([npatch]) = max_f max(|r_y|, |r_x|) of patch q.  2 <= t <= 512. */
int mc_xc_refine_update_patches(const int* peaks, const float* nb, float* shifts_px, int ref, int t, int npatch,
                                int q0, int nq, int H, int W, int under_px, float* max_r, void* stream);

/* ---- a11/a12/a13: per-frame shift post-processing ------------------------------- */
/* Sub-pixel parabola (rules Q4/Q5), wrap-around, outlier rejection
 * (estimate_motion_xc.py:538-627) and accumulation into field (2,t,gh,gw) [Angstrom]
 * for `nf` frames: pair index p = fi*npatch + g maps to frame frames[fi].
 * flags bit0 = sub_pixel_refinement, bit1 = outlier_rejection. */
int mc_field_accumulate(const int* peaks, const float* nb, const int* frames, int nf, int npatch,
                        int P, int t, float pixel_spacing, float outlier_threshold, int flags,
                        float* field, void* stream);
/* Savitzky-Golay (polyorder 1, mode "interp") along t for each (c,gy,gx), as
 * scipy.signal.savgol_filter at estimate_motion_xc.py:528-529; then (optional)
 * subtraction of the single global mean (xc.py:410).  Any window 3 <= window <= t, odd or
 * even (the reference reaches an even one as min(window|1, t) for even t: scipy then centres
 * the interior mean on x[i-w/2+1 .. i+w/2]).  field_out may alias field_in only if window < 3. */
int mc_field_smooth_center(const float* field_in, float* field_out, int t, int npatch, int window,
                           int subtract_mean, void* stream);

/* ---- a14/a16: cubic spline grids (csrc/field_tables.hip) -------------------------- */
/* Evaluate a (c,nt,nh,nw) uniform cubic spline grid on the tensor-product lattice
 * given by per-axis tap tables: for lattice coordinate i of an axis, 4 sample indices
 * idx_*[4*i+k] and 4 weights w_*[4*i+k] (basis weights of the Catmull-Rom or B-spline
 * matrix with the library's linear-extrapolation edge samples folded in by the host).
 * out[c][NT][NY][NX].  Replaces CubicCatmullRomGrid3d / CubicBSplineGrid3d as used by
 * deformation_field_utils.py:9-39,42-93,96-126. */
int mc_spline_lattice(const float* data, int c, int nt, int nh, int nw, const int* idx_t,
                      const float* w_t, int NT, const int* idx_y, const float* w_y, int NY,
                      const int* idx_x, const float* w_x, int NX, float* out, void* stream);

/* The same grid at npoints scattered (t, y, x) points -- evaluate_deformation_field on arbitrary
 * points (deformation_field_utils.py:9-39): per point 4 taps per axis, idx_*[4*i+k] / w_*[4*i+k];
 * out[npoints][c]. */
int mc_spline_points(const float* data, int c, int nt, int nh, int nw, const int* idx_t, const float* w_t,
                     const int* idx_y, const float* w_y, const int* idx_x, const float* w_x, int64_t npoints,
                     float* out, void* stream);

/* ---- a15/a17/a18: deformation-field warp ------------------------------------------
 * csrc/warp_field.hip (entry points, route rule, warp_field_plan / warp_field3 / warp_field_slow),
 * csrc/warp_field_fallback.hip (warp_main, warp_field2: fp32 frames only), csrc/field_tables.hip (the
 * lattice tables every route reads, mc_pixel_shifts*, mc_warp_scratch_bytes). */
/* lattice: (nframes, 2, GH, GW) Angstrom shifts on the 10x-oversampled lattice
 * (evaluate_deformation_field_at_t, correct_motion.py:67-72).  For every frame:
 * bicubic/reflection upsample to per-pixel shifts (get_pixel_shifts,
 * correct_motion.py:132-185), then bicubic/border resample of the frame at
 * pixel + shift/pixel_spacing with zero outside (_correct_frame + sample_image_2d,
 * correct_motion.py:81-129).  scratch: mc_warp_scratch_bytes() bytes, 16-byte aligned.
 * out_frames (nframes*h*w) and/or out_sum (h*w, OVERWRITTEN with the sum over the frames: the
 * caller need not clear it) may be NULL (not both).
 * The frames come in their storage type (MC_STORE_F32 / MC_STORE_F16; outputs stay fp32).  fp16 frames are
 * resampled straight from the fp16 bytes (half the HBM read) when w % 8 == 0, the frames are 16-byte aligned
 * and the lattice is sparse (32 pixel rows span <= 1.5 lattice cells); otherwise MC_ERR_UNSUPPORTED: widen
 * the stack and call again with MC_STORE_F32. */
int mc_warp_scratch_bytes(int nframes, int h, int w, int GH, int GW, int64_t* bytes /*host*/);
int mc_warp_frames_t(const void* frames, int storage, int nframes, int h, int w, const float* lattice,
                     int GH, int GW, float pixel_spacing, float* scratch, float* out_frames, float* out_sum,
                     void* stream);

/* N2: mc_warp_frames_t fed from the RAW movie: every sample is conditioned as raw * gain - mu[f] (gain (h,w)
 * fp32, mu from mc_raw_movie_stats) on its way into the resampler's window, so the outputs (fp32, same contract)
 * equal mc_warp_frames_t on the output of mc_condition_movie; outside the frame the result is the conditioned
 * domain's zero.  storage: MC_STORE_U8 (w % 16 == 0) or MC_STORE_I16 (w % 8 == 0); 16-byte aligned raw, the
 * sparse lattice of mc_warp_frames_t's fp16 path and h * w < 2^31; anything else is MC_ERR_UNSUPPORTED. */
int mc_warp_frames_raw(const void* raw, int storage, const float* gain, const float* mu, int nframes, int h, int w,
                       const float* lattice, int GH, int GW, float pixel_spacing, float* scratch, float* out_frames,
                       float* out_sum, void* stream);

/* mc_warp_frames_raw with the sum ACCUMULATED: out_sum (required) += this call's frame sum, each element by the one
 * lane that owns it (old + tile sum), then warp_field_slow adds its tile-frames as in mc_warp_frames_raw.  A movie
 * warped a chunk of frames at a time -- mc_warp_frames_raw for the first chunk, this for the rest, in stream order
 * -- sums to ((s_0 + s_1) + s_2) + ... of the per-chunk sums, reproducible bit for bit when no tile-frame takes
 * the slow kernel (with it, a chunk adds (old + fast) + slow).  NULL inputs or out_sum: MC_ERR_ARG before any
 * launch; shapes as mc_warp_frames_raw. */
int mc_warp_frames_raw_accumulate(const void* raw, int storage, const float* gain, const float* mu, int nframes, int h,
                                  int w, const float* lattice, int GH, int GW, float pixel_spacing, float* scratch,
                                  float* out_frames, float* out_sum, void* stream);

/* N2: the rigid warp (correct_motion for a (2,t,1,1) field, correct_motion.py:18-78) fed from the RAW movie:
 * every sample is conditioned as raw * gain - mu[f] on its way to the resampler (examples/ttMotion.py:90-121,
 * 180-199), so the result equals mc_warp_rigid_phase_t on the output of mc_condition_movie without that fp32 movie.
 * storage: MC_STORE_U8 or MC_STORE_I16; gain (h,w) fp32; mu from mc_raw_movie_stats; scratch / phase as
 * mc_warp_rigid_phase_t.  w % 4 == 0 and 16-byte aligned buffers, else MC_ERR_UNSUPPORTED. */
int mc_warp_rigid_raw(const void* raw, int storage, const float* gain, const float* mu, int nframes, int h, int w,
                      const float* shifts_px, float* scratch, float* out_frames, float* out_sum, int phase,
                      void* stream);

/* mc_warp_rigid_raw with the sum ACCUMULATED: out_sum (required) += this call's frame sum, each element by the one
 * lane that owns it (old + tile sum).  Chunks of a movie -- mc_warp_rigid_raw for the first, this for the rest, in
 * stream order -- sum to ((s_0 + s_1) + s_2) + ... bit for bit.  NULL inputs or out_sum: MC_ERR_ARG before any
 * launch; shapes and phase as mc_warp_rigid_raw. */
int mc_warp_rigid_raw_accumulate(const void* raw, int storage, const float* gain, const float* mu, int nframes, int h,
                                 int w, const float* shifts_px, float* scratch, float* out_frames, float* out_sum,
                                 int phase, void* stream);

/* The tail of the rigid movie pipeline in two launches: integer-peak shifts (t,2) px of estimate_global_motion ->
 * field (2,t) Angstrom (image_shifts_to_deformation_field, deformation_field_utils.py:129-162), the per-frame
 * shifts the corrector uses (the field's spline at the frame times, correct_motion.py:57-72, lattice point
 * (0,0), / pixel_spacing) and the weight tables of mc_warp_rigid_phase_t(phase 1) in `scratch`.  Results are
 * bit for bit those of mc_spline_lattice + mc_warp_rigid_phase_t. */
int mc_rigid_tables_from_shifts(const float* shifts, float pixel_spacing, const int* idx_t, const float* w_t,
                                const float* w_y, const float* w_x, int nframes, int h, int w, float* field,
                                float* shifts_px, float* scratch, void* stream);

/* Rigid special case of mc_warp_frames_t: a (2,nt,1,1) field gives each frame ONE shift,
 * shifts_px[f] = (sy, sx) in pixels (device).  The coordinate chain is then separable
 * and the resample is a regular 5x5 separable correlation (see warp_rigid.hip).  Same
 * outputs/contract as mc_warp_frames_t.  scratch: mc_warp_rigid_scratch_bytes().
 * phase 0 does it all; for callers that want to time or schedule the resampling kernel on its own, phase 1
 * fills the per-frame weight tables in `scratch` and phase 2 (same arguments) resamples.
 * The frames come in their storage type (MC_STORE_F32 / MC_STORE_F16; outputs stay fp32): fp16 frames are
 * DMA'd to LDS as they are and widened on the way to the registers (half the read bytes).  fp16 needs
 * w % 8 == 0 and 16-byte aligned frames / out_frames, else MC_ERR_UNSUPPORTED (widen and call again with
 * MC_STORE_F32). */
int mc_warp_rigid_scratch_bytes(int nframes, int h, int w, int64_t* bytes /*host*/);
int mc_warp_rigid_phase_t(const void* frames, int storage, int nframes, int h, int w, const float* shifts_px,
                          float* scratch, float* out_frames, float* out_sum, int phase, void* stream);

/* get_pixel_shifts (correct_motion.py:132-185) for one (2,GH,GW) lattice: out (h,w,2)
 * shifts in px.  scratch: mc_warp_scratch_bytes(1,h,w,GH,GW). */
int mc_pixel_shifts(const float* lattice, int GH, int GW, int h, int w, float pixel_spacing,
                    float* scratch, float* out, void* stream);
/* The same at caller-supplied coordinates -- the `pixel_grid` argument of get_pixel_shifts
 * (correct_motion.py:136,167-168) when it is not the identity grid: coords_yx (n,2) pixel
 * coordinates (y,x) of an (h,w) frame -> out (n,2) shifts in px. */
int mc_pixel_shifts_at(const float* lattice, int GH, int GW, int h, int w, float pixel_spacing,
                       const float* coords_yx, int64_t n, float* out, void* stream);

/* ---- full-spectrum transforms with a row-major spectrum -------------------------------------
 * What correct_motion_fast (correct_motion.py:484-496) and the exposure-filtered sum
 * (examples/ttMotion.py:331-351) run on for rows of W = 64 .. 8192 (powers of two), 5760 or 11520
 * columns and columns of H = 256 .. 4096 (powers of two), 4092 or 8184 rows -- any combination;
 * the K3 formats 4092 x 5760 and 8184 x 11520 are transformed by mixed-radix passes (radix 31, 11,
 * 8, 5, 3), no chirp-z.  MC_ERR_UNSUPPORTED otherwise: use the pruned-engine entry points below.
 * S[job][y][pitch] complex, pitch = mc_full_spectrum_pitch(W) = W/2 + 1 rounded up to 16.
 *   mc_full_rows_forward   rfft along x of njobs frames (origin src + job_off[j], rows row_stride
 *                          floats apart) -> S
 *   mc_full_cols_shift     per job: fft along y, * exp(-2 pi i (fy sy + fx sx)) * scale,
 *                          shifts[j] = (sy, sx) px, ifft along y, in place
 *   mc_full_rows_inverse   irfft along x (c2r, unscaled) of S -> real rows at out + out_off[j] */
int mc_full_spectrum_pitch(int W);
int mc_full_rows_forward(const float* src, const int64_t* job_off, int64_t row_stride, void* S,
                         const void* tw_row, int njobs, int H, int W, int pitch, void* stream);
int mc_full_cols_shift(void* S, const float* shifts, const void* tw_col, float scale, int njobs, int H, int W,
                       int pitch, void* stream);
/* Column-major copy of a chunk of row-major spectra, ST[job][kx][y] (kx <= W/2), for the accumulating
 * column passes (mc_full_cols_shift_sum_cm: contiguous columns instead of 8 bytes of every 128-byte line). */
int mc_full_transpose(const void* S, void* ST, int njobs, int H, int W, int pitch, void* stream);
int mc_full_rows_inverse(const void* S, float* out, const int64_t* out_off, int64_t out_stride,
                         const void* tw_row, int njobs, int H, int W, int pitch, void* stream);
/* Fused Fourier-shift sums (correct_motion_fast -> sum / dose_weighted_sum without the shifted frames):
 * the sums are linear, so sum_f irfft2(R_f X_f) = irfft2(sum_f R_f X_f), R_f = exp(-2 pi i (fy sy_f + fx sx_f)),
 * and the exposure-weighted sum of the shifted frames is irfft2(sum_f q_f R_f X_f) / sqrt(sum_f q_f^2).
 *   mc_full_rows_forward_raw  mc_full_rows_forward of raw frames: kind 0 u8 / 1 i16 (else MC_ERR_UNSUPPORTED),
 *                             sample = raw * gain - mu[j] rounded as mc_condition_movie rounds it (a product,
 *                             then a difference), so the spectra are bit for bit those of the conditioned
 *                             frames; frame j at element job_off[j] of raw, rows W samples apart; gain (H,W)
 *                             fp32, 8-byte aligned; raw 2- (u8) / 4-byte (i16) aligned.
 *   mc_full_rows_hot_correct  S[f][y][kx] += (r - v) exp(-2 pi i kx x / W), kx = 0 .. W/2, for the hot pixels
 *                             of an engine RawMovie's sorted list (keys = f H W + y W + x relative to the first
 *                             frame of S, rv = {replacement r, value v}) with frame0 <= f < frame0 + njobs:
 *                             after mc_full_rows_forward_raw the spectra are those of the movie with its hot
 *                             pixels replaced.  kx x is reduced mod W in integers; one writer per bin, in list
 *                             order (reproducible).
 *   mc_full_cols_shift_sum    per frame j of the nframes frames of S (frames frame0.. of total_frames): fft
 *                             along y, * exp(-2 pi i (fy sy + fx sx)) with shifts[j] = (sy, sx) px
 *                             (mc_full_cols_shift's angle), then accumulated over the frames: into P plainly,
 *                             into A weighted by the exposure filter q_f(k) (as mc_dose_accumulate), either or
 *                             both (NULL: not accumulated; at least one).  shifts == NULL: no phase ramp, the
 *                             exposure-weighted sum of the frames themselves -- valid with A alone (P set:
 *                             MC_ERR_ARG).  first: the sums start at zero, else add to what A / P hold; last: A
 *                             is scaled by scale / sqrt(sum_f q_f^2) over ALL frames, P by scale, and both are
 *                             transformed back along y (then mc_full_rows_inverse gives the sums).  A, P: H *
 *                             pitch complex.  The dose arguments are read only with A.  Both sums come from one
 *                             read of the spectra for H = 4096; other heights take one launch per sum.
 *   mc_full_cols_shift_sum_cm the same reading the column-major copy of mc_full_transpose (H = 4096, 4092,
 *                             8184). */
int mc_full_rows_forward_raw(const void* raw, int kind, const float* gain, const float* mu, const int64_t* job_off,
                             void* S, const void* tw_row, int njobs, int H, int W, int pitch, void* stream);
int mc_full_rows_hot_correct(const long long* keys, const float* rv, int64_t n, int frame0, int njobs, int H, int W,
                             void* S, int pitch, void* stream);
int mc_full_cols_shift_sum(const void* S, const float* shifts, int nframes, int frame0, int total_frames, void* A,
                           void* P, const void* tw_col, int H, int W, int pitch, float pixel_size, float pre_exposure,
                           float dose_per_frame, float voltage, int first, int last, float scale, void* stream);
int mc_full_cols_shift_sum_cm(const void* ST, const float* shifts, int nframes, int frame0, int total_frames, void* A,
                              void* P, const void* tw_col, int H, int W, int pitch, float pixel_size,
                              float pre_exposure, float dose_per_frame, float voltage, int first, int last, float scale,
                              void* stream);
/* Fourier cropping by 2 per axis (the "-FtBin 2" of production motion correction): with F = rfft2(x) of an
 * H x W frame, y = irfft2(G, (H/2, W/2)) of G = the rows -H/4 <= ky < H/4 (signed; the new Nyquist row from
 * the negative side) and columns 0 <= kx <= W/4 of F, scaled by 1 / ((H/2) (W/2)): the frame's sum is kept.
 *   mc_full_cols_crop  per job: columns kx <= W/4 of S (H x pitch; the others are never read): fft along y,
 *                      the kept rows * 1 / ((H/2)(W/2)), ifft along y at H/2 points -> S2 (H/2 x pitch2,
 *                      pitch2 = mc_full_spectrum_pitch(W/2); its padding columns hold nothing defined).
 *                      Between mc_full_rows_forward(_raw) at (H, W) and mc_full_rows_inverse at (H/2, W/2).
 *                      tw_col: the H-point table.  H and H/2 must both be column sizes above and W and W/2
 *                      row sizes (H = 512 .. 4096 or 8184; W = 128 .. 8192 or 11520), else MC_ERR_UNSUPPORTED. */
int mc_full_cols_crop(const void* S, void* S2, const void* tw_col, int njobs, int H, int W, int pitch, int pitch2,
                      void* stream);
/* Fourier cropping to a given size (H2, W2), both even, H2 < H, W2 <= W ("-FtBin 1.5", 3, 4/3; a K3 counting-mode
 * movie by 2): y = irfft2(G, (H2, W2)) of G = the rows -H2/2 <= ky < H2/2 (signed; the new Nyquist row from the
 * negative side) and columns 0 <= kx <= W2/2 of F, scaled by 1 / (H2 W2): the frame's sum is kept.
 *   mc_full_cols_crop_to  per job: columns kx <= W2/2 of S (H x pitch; the others are never read): fft along y, the
 *                      kept rows * 1 / (H2 W2), ifft along y at H2 points -> S2 (H2 x pitch2, pitch2 =
 *                      mc_full_spectrum_pitch(W2); its padding columns hold nothing defined).  Between
 *                      mc_full_rows_forward(_raw) at (H, W) and mc_full_rows_inverse at (H2, W2), which takes these
 *                      output sizes besides those above.  tw_col: the H-point table, tw_col2: the H2-point table.
 *                      (H, H2) is one of (512, 384), (4096, 3072), (4092, 2046), (8184, 5456), (8184, 2728); W a
 *                      row size above; W2 one too, or 2880, 3072, 3840 or 7680; else MC_ERR_UNSUPPORTED. */
int mc_full_cols_crop_to(const void* S, void* S2, const void* tw_col, const void* tw_col2, int njobs, int H, int W,
                         int H2, int W2, int pitch, int pitch2, void* stream);

/* correct_motion_fast (correct_motion.py:430-498): K3 variant multiplying spectrum
 * idx[p] by exp(-2*pi*i*(fy*sy+fx*sx)), shifts[p]=(sy,sx) px, then inverse columns. */
int mc_fourier_shift_cols_inverse(const void* S, const int* idx, const float* shifts, void* T2,
                                  const void* tw_col, float scale, int nframes,
                                  const mc_xc_geom* geom, void* stream);
/* K4 variant storing real rows: out + out_off[p] + y*out_stride. */
int mc_xc_rows_inverse_store(const void* T2, float* out, const int64_t* out_off,
                             int64_t out_stride, const void* tw_row, int nframes,
                             const mc_xc_geom* geom, void* stream);

/* ---- generic transform lengths (Bluestein): any even W (rows), any H (columns) ------ */
/* One line plan (host struct of device pointers): tw_m = exp(-2 pi i k/M) (M entries),
 * chirp = exp(-+ i pi j^2/n) (n entries; - for forward, + for inverse transforms),
 * bspec = FFT_M(wrapped conj(chirp)) / M (M entries); M = power of two >= 2n-1, <= 16384.
 * n is W/2 for the row functions and H for the column functions. */
typedef struct mc_xc_line {
  const void* tw_m;
  const void* chirp;
  const void* bspec;
  int M;
  int keep; /* 0: classic plan.  > 0 (mc_xcg_rows_forward only): output-pruned plan -- only
               outputs k < keep and k > n - keep are exact, which needs M >= n + 2 keep - 1 only;
               bspec = FFT_M of conj(chirp) wrapped over the offsets (-(n-1) - (keep-1) .. keep-1) / M */
} mc_xc_line;

/* Same contracts and layouts as mc_xc_rows_forward / mc_xc_cols_forward /
 * mc_xc_cols_inverse (+ Fourier-shift mode when `shifts` != NULL) /
 * mc_xc_rows_inverse_argmax (out == NULL) and mc_xc_rows_inverse_store (out != NULL),
 * without the power-of-two restriction: 4 <= W <= 16384 even or W <= 8191 odd (odd widths: the
 * row line plan has n = W points, one real sample each, instead of W / 2), 2 <= H <= 8192 (a row line plus
 * its staged bins must fit 160 KB of LDS: MC_ERR_ARG otherwise).
 * tw_row = exp(-2 pi i k / W), W entries. */
int mc_xcg_rows_forward(const float* src, const int64_t* job_off, int64_t row_stride,
                        const int* job_expo, const float* mask, const float* mean_rstd, void* T1,
                        const void* tw_row, const mc_xc_line* line, int njobs,
                        const mc_xc_geom* geom, void* stream);
/* N2: the K3-format rows (5760 / 11520 samples) from raw u8 / i16 bytes; see mc_xc_rows_forward_raw. */
int mc_xcg_rows_forward_raw(const void* raw, int storage, const float* gain, const int64_t* job_off,
                            int64_t row_stride, const float* mask, const float* job_sub, const float* mean_rstd,
                            void* T1, const void* tw_row, const mc_xc_line* line, int njobs, const mc_xc_geom* q,
                            void* stream);
int mc_xcg_cols_forward(const void* T1, const float* filt, void* S, const mc_xc_line* line,
                        int njobs, const mc_xc_geom* geom, void* stream);
int mc_xcg_cols_inverse(const void* S_cur, const int* cur_idx, const void* S_ref,
                        const int* ref_idx, const float* shifts, void* T2, const mc_xc_line* line,
                        float scale, int npairs, const mc_xc_geom* geom, void* stream);
int mc_xcg_rows_inverse(const void* T2, float* part_val, int* part_idx, int* peaks, float* shifts,
                        float* out, const int64_t* out_off, int64_t out_stride, const void* tw_row,
                        const mc_xc_line* line, int npairs, const mc_xc_geom* geom, void* stream);

/* K6 for any size (same contract as mc_xc_peak_neighbourhood, no twiddle table): the nine values
 * as direct sums over the kept columns of T2. */
int mc_xcg_peak_neighbourhood(const void* T2, const int* peaks, float* nb, int npairs,
                              const mc_xc_geom* geom, void* stream);

/* caller-side frame sum (examples/ttMotion.py:398): sum[h*w] = sum_t frames[t]. */
int mc_sum_frames(const float* frames, int nframes, int64_t hw, float* sum, void* stream);

/* Calibration from raw bytes: the per-pixel statistics a gain reference (gain = mean of the good pixels / pixel
 * mean) and a session-wide defect map (dead / hot / stuck pixels) are estimated from, as relion_estimate_gain
 * and MotionCor2's gain tools do where the reference's example loads a file (examples/ttMotion.py:40-121).
 * raw: contiguous (t, h, w) movie, u8 (is_i16 == 0) or i16 (is_i16 == 1).  sum, sumsq: (h, w) 64-bit
 * accumulators; the call ADDS sum_f v and sum_f v^2 to them, exactly, so repeated calls accumulate a session
 * (zero them first; the caller keeps sumsq below 2^63: 255^2 n for u8, 2^30 n for i16 after n frames).  One read
 * of the movie's bytes, nothing written per frame; any h, w, t >= 1 (rows of whole 16-byte pieces at 16-byte
 * addresses take the vector path, everything else one load per pixel with the same results). */
int mc_raw_pixel_sums(const void* raw, int is_i16, int t, int h, int w, long long* sum, unsigned long long* sumsq,
                      void* stream);

/* Rolling frame-group sums of a raw movie (MotionCor2 -Group, RELION --group_frames): out (t, h, w) int16, frame i
 * = the sum of the input frames max(0, i - lo) .. min(t - 1, i + hi) with lo = (group - 1) / 2, hi = group / 2:
 * the centred window of `group` frames clipped at the ends of the movie; group == 1 widens the movie.  raw:
 * contiguous (t, h, w), storage MC_STORE_U8 or MC_STORE_I16 (anything else: MC_ERR_UNSUPPORTED).  Exact integers:
 * a u8 window of min(group, t) <= 128 frames cannot leave int16; an i16 window may hold up to 32768 frames (longer
 * windows of either kind: MC_ERR_UNSUPPORTED) and sets *overflow = 1 (device memory, zeroed by the caller) when a
 * window sum leaves [-32768, 32767] -- the output of such a call is unspecified.  One read of the movie plus the
 * re-read of each window's trailing frame, one write of the output; any h, w, t >= 1 (rows of whole 16-byte pieces
 * at 16-byte addresses, input and output, take the vector path, everything else one load per pixel with the same
 * results). */
int mc_raw_group_frames(const void* raw, int storage, int t, int h, int w, int group, short* out, int* overflow,
                        void* stream);

/* Detector defects filled from the session's defect map (MotionCor2 -DefectFile / -DefectMap, RELION
 * --defect_file), in a raw movie and in its gain reference.  map: (h, w) bytes, non-zero = defect.  pixels: the n
 * defect pixels' linear indices y * w + x in row-major (ascending) order; j is a pixel's place in that list.  reach:
 * 1 .. 16.  donors: (n, 8 * reach) ints, counts: n ints.  h * w must fit an int.
 *
 * mc_defect_donors writes the tables: with the ring at Chebyshev distance r around a defect = the pixels of
 * max(|dy|, |dx|) == r inside the frame, r_j is the smallest r in 1 .. reach whose ring holds a good pixel;
 * donors[j][0 .. counts[j]) are the good pixels of that one ring in row-major order and the rest of the row is -1.
 * counts[j] == 0: no good pixel within reach (the caller's error to report).
 *
 * mc_raw_fill_defects fills a contiguous (t, h, w) movie of elem_bytes = 1, 2 or 4 bytes per element IN PLACE:
 * movie[f][pixels[j]] = movie[f][donors[j][k]], the element's bits untouched, with the pick (uint32, wrapping)
 *   x = seed ^ (f * 0x9E3779B1) ^ (j * 0x85EBCA77);
 *   x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16;   k = ((uint64)x * counts[j]) >> 32.
 * Donors are good pixels and no good pixel is written: nothing else of the movie changes, and the call has no
 * races.  A row with counts[j] == 0 is left as it is.
 *
 * mc_gain_fill_defects: gain[pixels[j]] = (float)(sum_k (double)gain[donors[j][k]] / counts[j]), the sum in table
 * order, in place; every other gain stays.
 *
 * MC_ERR_ARG for null pointers, sizes < 1, reach outside 1 .. 16, elem_bytes not 1, 2 or 4 and a movie or gain
 * that is not aligned to its element; n == 0 is MC_OK without a launch (the tables may then be null). */
int mc_defect_donors(const unsigned char* map, int h, int w, const int* pixels, int n, int reach, int* donors,
                     int* counts, void* stream);
int mc_raw_fill_defects(void* movie, int elem_bytes, int t, int h, int w, const int* pixels, const int* donors,
                        const int* counts, int n, int reach, unsigned seed, void* stream);
int mc_gain_fill_defects(float* gain, int h, int w, const int* pixels, const int* donors, const int* counts, int n,
                         int reach, void* stream);

/* EER event movies (Falcon 4 / 4i) rendered into a raw u8 movie: out (n_frames / group, up h, up w) bytes, frame k =
 * the per-pixel event count of the input frames k group .. k group + group - 1 (the trailing n_frames % group frames
 * are decoded and checked but fill no output frame).  data: the device buffer that holds the strips, data_bytes long;
 * offsets / nbytes: HOST arrays of n_frames entries, frame f's strip is data[offsets[f] .. offsets[f] + nbytes[f]).
 * The codec rule (7-bit runs, 4-bit sub-pixel codes; csrc/eer.h) places an event of the h x w detector at (y, x) for
 * upsampling 1 and at (2 y + ((s >> 3) & 1), 2 x + ((s >> 1) & 1)) for upsampling 2.  A count is at most group <= 255:
 * nothing saturates.  final_n, events: n_frames ints each (device): the pixel count n at which frame f's decoding
 * stopped (== h * w for a well-formed stream, anything else is the caller's error to report) and its events.
 * seg_bytes: the segment size of the parallel parse, 64, 128 or 256.  scratch (device, 8-byte aligned) must hold
 *   scratch_bytes >= 24 * n_frames + 52 * sum_f ceil(nbytes[f] / seg_bytes).
 * No kernel reads a byte outside a frame's own strip, whatever the bits say.  The call zeroes out on the stream,
 * copies the frame table to the device (it returns after that copy) and launches three kernels.
 * Before anything is launched: MC_ERR_ARG for null pointers, sizes < 1, group < 1, n_frames < group, a strip outside
 * the buffer, misaligned out / final_n / events / scratch, a scratch that is too small, and an rle_bits or upsampling
 * that names no format; MC_ERR_UNSUPPORTED for rle_bits 8 (compression 65000), upsampling 4, group > 255, h * w >=
 * 2^31, a strip of 2^28 bytes or more, 2^31 segments or more, up w % 4 != 0 and any other seg_bytes. */
int mc_eer_render(const unsigned char* data, long long data_bytes, const long long* offsets, const long long* nbytes,
                  int n_frames, int h, int w, int rle_bits, int upsampling, int group, int seg_bytes,
                  unsigned char* out, int* final_n, int* events, void* scratch, long long scratch_bytes, void* stream);

/* ---- estimate_local_motion (estimate_motion_optimizer.py:28-439): loss + gradient ------
 * The reference rebuilds, every iteration and for every patch, rfftn(patch * mask), the
 * Fourier shift by the spline-predicted shifts, the band-pass and B-factor filters, the
 * leave-one-out reference and the loss (:361-417, :466-514, :611-671), and differentiates
 * it with autograd.  Here the masked + filtered patch spectra are computed once (pruned,
 * layout of mc_xc_cols_forward: (npatch * t jobs, nkx, nky) complex, job = patch * t +
 * frame) and an iteration is two passes over them.
 * mc_local_loss_sums: for every patch b, bin tile and frame f (partial: (npatch, ntiles,
 * t, 6) floats, to be summed over the tiles by the caller):
 *   [0] sum h fy Im(conj(S) G_f)   [1] same with fx   [2] sum h |t G_f - S|^2
 *   [3] sum h Re(G_f conj(S - G_f))   [4] sum h |S - G_f|^2   [5] sum h |G_f|^2
 * with G_f = P_f exp(-2 pi i (fy sy_f + fx sx_f)), S = sum_f G_f, shifts_px (npatch, t,
 * 2) = (y, x) pixels, fy (nky) / fx (nkx) = the bins' frequencies in cycles/pixel, hx
 * (nkx) = weight of column kx (NULL = 1; Hermitian multiplicities for the real-space
 * losses).  Loss values and shift gradients of "mse", "cc" follow from these sums
 * (csrc/local_motion.hip header); "ncc" needs mc_local_ncc_grad with ab (npatch, t, 2) =
 * (dL/dn_f, dL/dey_f) -> partial (npatch, ntiles, t, 2) = sum h f{y,x} Im(V_f G_f).
 * 1 <= t <= 512. */
int mc_local_loss_tiles(int nkx, int nky, int* ntiles);
int mc_local_loss_sums(const void* spectra, const float* shifts_px, const float* fy, const float* fx,
                       const float* hx, int npatch, int t, int nkx, int nky, float* partial,
                       void* stream);
int mc_local_ncc_grad(const void* spectra, const float* shifts_px, const float* fy, const float* fx,
                      const float* hx, const float* ab, int npatch, int t, int nkx, int nky,
                      float* partial, void* stream);

/* correct_motion_fast (correct_motion.py:484-496) for frames whose full spectrum does not fit one
 * row line (more than ~8190 columns): the frame's even and odd columns are transformed as two
 * (H, W/2) frames (mc_xcg_rows_forward / mc_xcg_cols_forward, full geometry) into S -- (2 nframes,
 * W/4 + 1, H) complex, job j = even columns of frame j, job j + nframes = odd columns -- and this
 * call applies, in place, the radix-2 butterfly to the bins of the full spectrum, the phase ramp
 * exp(-2 pi i (fy sy + fx sx)) at each bin's own frequency (shifts_px (nframes, 2) = (y, x)), and the
 * inverse butterfly; the two halves are then inverse-transformed with zero shifts and interleaved.
 * W % 4 == 0; nkx must be W/4 + 1. */
int mc_polyphase_fourier_shift(void* S, const float* shifts_px, int nframes, int nkx, int H, int W,
                               void* stream);
/* mc_dose_accumulate in the same form: S holds the spectra of the even (jobs 0..nframes-1) and odd
 * (jobs nframes..2 nframes-1) columns of a chunk of frames; A (2, W/4 + 1, H) complex accumulates
 * the weighted butterfly outputs and, on the last chunk, becomes the spectra of the even / odd
 * columns of the exposure-weighted sum (inverse-transform both with zero shifts and interleave). */
int mc_polyphase_dose_accumulate(const void* S, int nframes, int frame0, int total_frames, void* A,
                                 int nkx, int H, int W, float pixel_size, float pre_exposure,
                                 float dose_per_frame, float voltage, int first, int last,
                                 void* stream);

/* TIFF strips -> a raw movie: the strips of a multi-page TIFF, LZW-coded (compression 5, TIFF 6.0: MSB-first codes,
 * early change; the rule is stated in csrc/tiff_lzw.h) or stored (compression 1), decoded into the contiguous
 * (n_frames, h, row_bytes) bytes of `out`; row_bytes = w * bytes per sample, the sample type is the caller's view.
 * data: the buffer that holds every strip (device), data_bytes its size.  offsets, nbytes (host): n_frames *
 * strips_per_frame entries each, frame-major: strip k of frame f covers rows k * rows_per_strip .. of that frame and
 * lies at offsets[f * strips_per_frame + k]; strips may lie anywhere in the buffer, in any order.  produced (device):
 * one int per strip, the bytes written for it; anything but the size of its rows means a strip that ended early
 * (cut short, malformed), the caller's error to report.  A strip reads its own bytes and writes its own rows only,
 * whatever its bits say; bytes a strip holds beyond its rows are ignored.  scratch: 16 bytes per strip (device,
 * 8-byte aligned).  One wavefront per strip.
 * Before anything is launched: MC_ERR_ARG for null pointers, sizes < 1, rows_per_strip > h, a strips_per_frame other
 * than ceil(h / rows_per_strip), a strip outside the buffer, a misaligned produced / scratch and a scratch that is
 * too small; MC_ERR_UNSUPPORTED for any other compression, a strip whose decoded size is 2^31 bytes or more and 2^31
 * strips or more. */
int mc_tiff_decode(const unsigned char* data, long long data_bytes, const long long* offsets, const long long* nbytes,
                   int n_frames, int strips_per_frame, int h, int row_bytes, int rows_per_strip, int compression,
                   unsigned char* out, int* produced, void* scratch, long long scratch_bytes, void* stream);

/* A raw movie -> TIFF LZW strips (compression 5; the encoder rule -- a leading Clear, greedy longest match, Clear once
 * the decoder's next code reaches 4093, EOI -- and the size bound are stated in csrc/tiff_lzw_encode.h).
 * mc_tiff_encode_slot_bytes: *slot_bytes = an upper bound, a multiple of 16, on the stream of a strip of strip_bytes
 * bytes.  MC_ERR_ARG for a null pointer or a negative size, MC_ERR_UNSUPPORTED for 2^31 bytes or more.
 * mc_tiff_encode: src (device) is the contiguous (n_frames, h, row_bytes) bytes of the movie; strip k of frame f is
 * rows k * rows_per_strip .. of that frame (the last strip of a frame holds the rest), and strip s of the frame-major
 * list is encoded, one wavefront per strip, into slots[s * slot_bytes ..] (device; slots_bytes is the whole buffer's
 * size) and gives produced[s] (device, 64-bit), the bytes of its stream.  A strip's wavefront reads its rows only and
 * writes its slot only, never more than slot_bytes of it.  Before anything is launched: MC_ERR_ARG for null pointers,
 * sizes < 1, rows_per_strip > h, a produced not aligned to 8 or a slots not aligned to 16 bytes, a slot_bytes that is
 * no multiple of 16 or below mc_tiff_encode_slot_bytes(rows_per_strip * row_bytes), and a slots_bytes below n_frames
 * * ceil(h / rows_per_strip) * slot_bytes; MC_ERR_UNSUPPORTED for a compression other than 5 (stored strips are the
 * movie's bytes), a strip of 2^31 bytes or more and 2^31 strips or more.
 * mc_tiff_pack: payload[offsets[s] .. offsets[s] + produced[s]) = slots[s * slot_bytes ..] for the n_strips strips
 * (all device; offsets, 64-bit, is the exclusive scan of produced).  Nothing is written outside that range, clipped to
 * slot_bytes and to payload_bytes, whatever the two arrays hold.  MC_ERR_ARG for null pointers, sizes < 1 and an
 * offsets or produced not aligned to 8 bytes; MC_ERR_UNSUPPORTED for 2^31 strips or more. */
int mc_tiff_encode_slot_bytes(long long strip_bytes, long long* slot_bytes /*host*/);
int mc_tiff_encode(const unsigned char* src, int n_frames, int h, int row_bytes, int rows_per_strip, int compression,
                   unsigned char* slots, long long slot_bytes, long long slots_bytes, long long* produced,
                   void* stream);
int mc_tiff_pack(const unsigned char* slots, long long slot_bytes, const long long* offsets, const long long* produced,
                 long long n_strips, unsigned char* payload, long long payload_bytes, void* stream);

/* MRC2014 sample rows -> a raw movie: the t * h rows of an MRC file's payload, which starts `offset` bytes into
 * `data` (device, data_bytes long; the payload has no alignment), decoded into the contiguous (t, h, w) elements of
 * `out`.  mode 0: 8-bit, copied to uint8 when unsigned_bytes, else widened from signed to int16; modes 1, 6, 12:
 * 2-byte samples copied as they are (byte-swapped when swap); mode 2: float32 (4-byte swap when swap); mode 101:
 * 4-bit samples, a row of (w + 1) / 2 bytes, pixel 2k the low and pixel 2k + 1 the high nibble of byte k, to uint8
 * 0..15 (the rule is stated in csrc/mrc.h).  swap is ignored for 1-byte and 4-bit samples, unsigned_bytes for every
 * mode but 0.  flip_rows: row r of every output frame is row h - 1 - r of the file's frame.  A row's threads read
 * the bytes of that row only and write its elements only; rows are cut at the 16-byte boundaries of the source.
 * Before anything is launched: MC_ERR_ARG for null pointers, data == out, sizes < 1, a negative offset or
 * data_bytes, offset + t * h * row_bytes > data_bytes, a mode other than 0, 1, 2, 6, 12, 101, a swap, unsigned_bytes
 * or flip_rows other than 0 or 1 and an `out` misaligned for its element type; MC_ERR_UNSUPPORTED for
 * h * w >= 2^31. */
int mc_mrc_decode(const unsigned char* data, long long data_bytes, long long offset, int t, int h, int w, int mode,
                  int swap, int unsigned_bytes, int flip_rows, void* out, void* stream);

/* A raw movie -> MRC2014 sample rows and the statistics the MRC header asks for, in one pass: the inverse of
 * mc_mrc_decode for the integer types (the rule is stated in csrc/mrc_encode.h).  movie (device): the contiguous
 * (t, h, w) elements of elem_bytes = 1 (uint8) or 2 (int16).  mode: uint8 -> 0 (the bytes) or 101 (4-bit, values
 * 0..15); int16 -> 1 (the two bytes, little-endian), 6 (the same bytes, values 0..32767), 0 (one signed byte, values
 * -128..127) or 101.  A mode-101 row is (w + 1) / 2 bytes, pixel 2k the low and pixel 2k + 1 the high nibble of byte
 * k, the last high nibble of a row of odd w written as 0.  flip_rows: row r of every payload frame is row h - 1 - r of
 * the movie's frame.  payload (device, any alignment, payload_bytes long): t * h rows one after the other, written
 * whole bytes at a time, each byte by one thread; nothing beyond them is written.  stats (device, 8-byte aligned):
 * t x 5 64-bit integers per frame, {min, max, sum, sum of squares of the samples as read, samples outside the mode's
 * range}, exact and independent of scheduling; a sample out of range is written as its low bits masked to the field,
 * and the caller refuses the movie.  scratch (device, 8-byte aligned): scratch_bytes >= t * B * 40 with B =
 * min(1024, ceil(h * (w * elem_bytes / 16 + 2) / 256)), the workgroups of a frame (integer division inside).
 * Before anything is launched: MC_ERR_ARG for null pointers, movie == payload, sizes < 1, a flip_rows other than 0
 * or 1, h * w >= 2^31, a payload_bytes below t * h * the row's bytes, a movie misaligned for its element, a stats or
 * scratch not aligned to 8 bytes and a scratch that is too small; MC_ERR_UNSUPPORTED for an (elem_bytes, mode) pair
 * outside the list above. */
int mc_mrc_encode(const void* movie, int elem_bytes, int t, int h, int w, int mode, int flip_rows,
                  unsigned char* payload, long long payload_bytes, long long* stats, void* scratch,
                  long long scratch_bytes, void* stream);

/* Quarter turns and flips of n images: out = numpy.rot90(in, rot90, axes=(-2, -1)) (counter-clockwise), then
 * flip 1 ("ud": the rows' order reversed) or flip 2 ("lr": every row reversed), flip 0 for neither.  in: (n, h, w)
 * elements of elem_bytes = 1, 2 or 4 bytes (device); out: (n, h, w) for even rot90, (n, w, h) for odd, the same
 * element size, a different buffer.  Exact: elements are moved.  Even rot90 is a row copy, odd a tiled transpose
 * through LDS (128-byte x 128-byte tiles); the flip is folded into the destination index.
 * Before anything is launched: MC_ERR_ARG for null pointers, in == out, sizes < 1, an elem_bytes other than 1, 2, 4,
 * rot90 outside 0..3, flip outside 0..2 and an `in` or `out` misaligned for its element size; MC_ERR_UNSUPPORTED for
 * h * w >= 2^31. */
int mc_raw_orient(const void* in, int elem_bytes, int n, int h, int w, int rot90, int flip, void* out, void* stream);

/* nframes frames resampled through a 2 x 2 linear map about their centre, bicubic (magnification distortion
 * correction; the rule is stated in csrc/affine_resample.h).  src (device): contiguous (nframes, h, w) samples of
 * `storage` MC_STORE_F32 or MC_STORE_F16; dst (device): (nframes, h, w) fp32, a buffer that does not overlap src.
 * m (host, read before the call returns): m00, m01, m10, m11 in (y, x) order.  Output pixel (y, x) samples the frame at
 * py = (cy + m00 (y - cy)) + m01 (x - cx), px = (cx + m10 (y - cy)) + m11 (x - cx), cy = h / 2, cx = w / 2, evaluated
 * in float64 on the device; a position outside [0, h - 1] x [0, w - 1] gives fill_value, any other the 4 x 4 Keys
 * (A = -0.75) sum in fp32 with the fractions rounded to fp32 and taps outside the frame clamped to its edge.  One
 * 64 x 64 output tile per workgroup, its source window staged in LDS; no scratch, no atomics, results independent of
 * scheduling; the identity returns the input's values exactly.
 * Before anything is launched: MC_ERR_ARG for null pointers, nframes < 1, h < 4 or w < 4, a value of m that is not
 * finite, a row sum |m00| + |m01| or |m10| + |m11| outside [0.8, 1.25] (the bound the window's size rests on), a
 * misaligned src or dst and byte ranges of src and dst that overlap; MC_ERR_UNSUPPORTED for another storage and for
 * h * w >= 2^31. */
int mc_affine_resample(const void* src, int storage, int nframes, int h, int w, const double m[4] /* host */,
                       float fill_value, float* dst, void* stream);

/* The aligned sum of a movie with the magnification map folded into the rigid warp: ONE bicubic resampling per frame
 * (the rule is stated in csrc/affine_warp_sum.h over csrc/affine_resample.h).  src (device): contiguous (t, h, w)
 * samples of `storage`, any MC_STORE_* kind; gain (h, w) fp32 and mu (t) fp32 from mc_raw_movie_stats (device) are
 * read for MC_STORE_U8 / MC_STORE_I16 only, whose samples enter as fp32(raw) * gain - mu[f], product and difference
 * rounded separately as mc_condition_movie rounds them.  m (host, read before the call returns): m00, m01, m10, m11 in
 * (y, x) order; shifts (device): (t, 2) fp32 pixel shifts (y, x) of the frames.  Output pixel (y, x) samples frame f
 * at py = ((cy + m00 (y - cy)) + m01 (x - cx)) + shifts[f][0], px likewise with shifts[f][1], in float64 on the device;
 * a position outside [0, h - 1] x [0, w - 1] contributes exactly 0, any other the 4 x 4 Keys (A = -0.75) sum of
 * mc_affine_resample.  sum (h, w) fp32 = ((0 + v_0) + v_1) + ... + v_{t-1}, one accumulator per pixel in registers;
 * frames: NULL, or (t, h, w) fp32 that receives every v_f.  One 64 x 64 output tile per workgroup, the frames in a loop,
 * each frame's source window staged in LDS; no scratch, no atomics, bits independent of the launch geometry.
 * Before anything is launched: MC_ERR_ARG for a null src, m, shifts or sum, t < 1, h < 4 or w < 4, a storage outside
 * 0 .. 3, a null gain or mu with MC_STORE_U8 / MC_STORE_I16, an m that mc_affine_resample refuses, a misaligned
 * pointer and outputs that overlap src or each other; MC_ERR_UNSUPPORTED for h * w >= 2^31. */
int mc_affine_warp_sum(const void* src, int storage, const float* gain, const float* mu, int t, int h, int w,
                       const double* m /* host: 4 doubles */, const float* shifts, float* sum, float* frames, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MCORR_H */
