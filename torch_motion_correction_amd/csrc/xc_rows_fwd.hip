// K1 of the pruned cross-correlation engine (xc_common.h has the map of the passes): forward row transforms,
//   gather + (x - mean) * rstd * mask^e -> real FFT(W) -> first nkx bins -> T1[job][kx][ysupport]
// by three engines, one object each -- a workgroup per row group (any power-of-two width, xc_rows_fwd_wg.hip), a
// wavefront per 4096-sample row (xc_rows_fwd_wave.hip) and a wavefront per 1024-sample patch row
// (xc_rows_fwd_wave512.hip).  Here: the entry points, the rules that route a job to an engine, the kernels of
// the fused frame statistics, and the hot-pixel correction of a raw movie's T1.
#include "xc_rows_fwd.h"

// Provisional mean of the fused-statistics path: m0 = {mean of n samples, 1, 1} by ONE
// workgroup (any value near the true mean keeps the linear fix-up free of cancellation).
template <typename T>
__global__ __launch_bounds__(256) void xc_provisional_mean_kernel(const T* __restrict__ x, int n,
                                                                  float* __restrict__ m0) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)(float)x[i];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
  __shared__ double part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    m0[0] = (float)(((part[0] + part[1]) + (part[2] + part[3])) / (double)n);
    m0[1] = 1.f;
    m0[2] = 1.f;
  }
}

// (sum, sumsq) of (x - m0) over `count` samples, spread over XC_STAT_SLOTS accumulators
// -> fix = {mean - m0, 1/std}, out3 = {mean, 1/std, std}  (unbiased std, as
// torch.std_mean, utils.py:81)
__global__ void xc_stats_finalize(const double* __restrict__ acc_slots, double count,
                                  const float* __restrict__ m0, float* __restrict__ fix,
                                  float* __restrict__ out3) {
  double acc[2] = {0.0, 0.0};
  for (int s = 0; s < XC_STAT_SLOTS; ++s) {
    acc[0] += acc_slots[2 * s];
    acc[1] += acc_slots[2 * s + 1];
  }
  const double dm = acc[0] / count;
  double var = (acc[1] - acc[0] * acc[0] / count) / (count - 1.0);
  if (var < 0) var = 0;
  const float stdf = (float)sqrt(var);
  fix[0] = (float)dm;
  fix[1] = 1.0f / stdf;
  out3[0] = (float)((double)m0[0] + dm);
  out3[1] = 1.0f / stdf;
  out3[2] = stdf;
}

// ------------------------------------------------------------------ K1 from raw frames: hot pixels
// K1 (raw) transformed A = (v - sub_f) * rstd * mask; a hot pixel's sample is
// (r - sub_f) * rstd * mask, so every kept bin of its row gains  dA * exp(-2 pi i kx x / W),
// dA = (r - v) * rstd * mask(y, x)  (the forward rfft convention of K1: no scale, negative exponent).
// One workgroup per (frame, row) segment of the sorted list -- the workgroup of the segment's first entry;
// the others return at once -- so every T1 element is written by one workgroup, in list order.
__global__ __launch_bounds__(256) void xc_rows_hot_fix(const long long* __restrict__ keys, const float2* __restrict__ rv,
                                                       int64_t n, int frame0, int njobs, int h, int w,
                                                       const float* __restrict__ mask,
                                                       const float* __restrict__ mean_rstd, cfloat* __restrict__ T1,
                                                       int W, int nkx, int y0, int ny) {
#pragma clang fp contract(off)  // dA and the sums in a fixed operation order (tests/hot_reference.py)
  const int64_t e0 = blockIdx.x;
  if (e0 >= n) return;
  const long long seg = keys[e0] / w;  // f * h + y
  if (e0 > 0 && keys[e0 - 1] / w == seg) return;
  const int f = (int)(seg / h), y = (int)(seg - (long long)f * h);
  if (f < frame0 || f >= frame0 + njobs || y < y0 || y >= y0 + ny) return;
  const float rstd = mean_rstd[1];
  cfloat* col = T1 + (int64_t)(f - frame0) * nkx * ny + (y - y0);
  for (int kx = threadIdx.x; kx < nkx; kx += 256) {
    float ar = 0.f, ai = 0.f;
    for (int64_t e = e0; e < n && keys[e] / w == seg; ++e) {
      const int x = (int)(keys[e] - seg * w);
      const float m = mask ? mask[(int64_t)y * w + x] : 1.f;
      if (m == 0.f) continue;
      const float2 p = rv[e];
      const float dA = (p.x - p.y) * rstd * m;
      const int ph = (int)(((int64_t)kx * x) % W);  // exact phase index; the angle in revolutions ph / W
      const float rev = (float)ph / (float)W;        // in [0, 1): v_sin / v_cos take revolutions
      ar += dA * __builtin_amdgcn_cosf(rev);
      ai -= dA * __builtin_amdgcn_sinf(rev);
    }
    cfloat* o = col + (int64_t)kx * ny;
    o->x += ar;
    o->y += ai;
  }
}

// ------------------------------------------------------------------ host dispatch
// mc_xc_row_engine(): 0 = automatic (wave-per-row kernel whenever the shape fits),
// 1 = always the workgroup-per-row kernels (A/B timing and cross-checks of the engines).
static int g_row_engine = 0;

// Whole-frame jobs: the wave-per-row engine or the workgroup-per-row engine.  The wave engine transforms rows of
// 4096 samples with at most 512 kept bins in whole rounds of 8 rows, and of those it takes
//  - fp32 / fp16 jobs (raw == 0) with one mask, no per-job exponent and a statistics box of whole 256-sample
//    chunks.  It reads samples and mask rows with 16-byte loads (4 fp32 samples: row_stride % 4); job_off[]
//    lives on the device: callers of the C ABI keep it a multiple of 4 floats whenever W == 4096 (whole frames:
//    f * h * w; documented in mcorr.h).  mc_xc_row_engine(1) sends these jobs to the workgroup engine too.  fp16
//    samples: only the wave engine reads them; anything else is K1_NONE (MC_ERR_UNSUPPORTED: the caller widens
//    the stack once).
//  - raw u8 / i16 jobs (raw != 0), whose entry has checked the mask: 16-byte aligned raw, gain and mask and rows
//    of whole 8-sample units (row_stride % 8: 8 bytes of u8, 16 of i16 -- the unit mcorr.h documents for this
//    entry and for the statistics and hot-pixel passes that come before it).  mc_xc_row_engine does not reach them.
enum K1Engine { K1_WAVE, K1_WG, K1_NONE };
static K1Engine k1_route(const XcGeom& g, int raw, bool half, const void* src, const float* gain, const float* mask,
                         const int* job_expo, int64_t row_stride, const XcBox& b, bool stats) {
  const bool shape = g.W == 2 * WF_N && g.nkx <= 512 && (g.ny % 8) == 0;
  const bool aligned16 = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(gain) |
                           reinterpret_cast<uintptr_t>(mask)) & 15) == 0;  // (gain: NULL unless raw)
  if (raw) return shape && aligned16 && (row_stride & 7) == 0 ? K1_WAVE : K1_WG;
  const bool wave = shape && mask && !job_expo && aligned16 && (row_stride & 3) == 0 &&
                    (!stats || ((b.wl | b.wu) & 255) == 0);
  if (half && !wave) return K1_NONE;
  return wave && g_row_engine != 1 ? K1_WAVE : K1_WG;
}

// The variant of the wave-per-row kernel for a job k1_route sent there
static K1WaveVariant k1_wave_variant(const XcGeom& g, int raw, bool half, const int* row_chord) {
  // square 4096 frames: the first and the last 256-sample chunk of a row lie outside the mask's support
  const bool inner = g.x0 >= 256 && g.x0 <= 512 && g.x1 >= 3584 && g.x1 <= 3840;
  // fp16 and raw storage: the general variant (all 16 chunks, per-row chord clamp when given)
  if (half) return K1WaveVariant{g.nkx <= 256, K1_LOADS_HALF};
  if (raw || !inner) return K1WaveVariant{g.nkx <= 256, K1_LOADS_ALL};
  return K1WaveVariant{g.nkx <= 256, row_chord ? K1_LOADS_INNER_CHORD : K1_LOADS_INNER};
}

// Patch rows the wave-per-1024-sample-row engine takes: 1024 samples, at most 128 kept bins, whole rounds of 8 rows,
// mask rows read as 8-byte pairs
static bool wave512_shape(const XcGeom& g, const float* mask) {
  return g.W == 2 * WF5_N && g.nkx <= 128 && (g.ny % 8) == 0 && (reinterpret_cast<uintptr_t>(mask) & 7) == 0;
}

extern "C" {

int mc_xc_row_engine(int mode) {
  if (mode < 0 || mode > 1) return MC_ERR_ARG;
  g_row_engine = mode;
  return MC_OK;
}

int mc_xc_rows_lds_bytes(const mc_xc_geom* q) {
  XcGeom g;
  int rc = geom_from(q, &g, true, false);
  if (rc) return rc;
  return (int)rows_lds_bytes(g.W / 2, g);
}

static int rows_forward_impl(const float* src, const int64_t* job_off, int64_t row_stride,
                             const int* job_expo, const float* mask, const float* mean_rstd,
                             void* T1, const void* tw_row, int njobs, const mc_xc_geom* q,
                             const XcBox* box, double* stats_acc, void* stream,
                             const int* row_chord = nullptr, bool half = false) {
  XcGeom g;
  int rc = geom_from(q, &g, true, false);
  if (rc) return rc;
  if (!src || !job_off || !T1 || !tw_row || njobs < 1) return MC_ERR_ARG;
  const XcBox b = box ? *box : XcBox{0, 0, 0, 0};
  switch (k1_route(g, 0, half, src, nullptr, mask, job_expo, row_stride, b, stats_acc != nullptr)) {
    case K1_NONE: return MC_ERR_UNSUPPORTED;
    case K1_WG:
      return k1_wg_launch(0, src, job_off, row_stride, job_expo, mask, mean_rstd, T1, tw_row, njobs, g, b, stats_acc,
                          nullptr, nullptr, stream);
    default:
      return k1_wave_launch(k1_wave_variant(g, 0, half, row_chord), 0, src, job_off, row_stride, mask, mean_rstd, T1,
                            tw_row, njobs, g, b, stats_acc, row_chord, nullptr, nullptr, stream);
  }
}

int mc_xc_rows_forward_dual_t(const void* src, int storage, const int64_t* job_off, int64_t row_stride,
                              const int* expo_a, const int* expo_b, const float* mask,
                              const float* mean_rstd, void* T1a, void* T1b, const void* tw_row,
                              int njobs, const mc_xc_geom* q, const int* row_chord, void* stream) {
  if (storage != MC_STORE_F32 && storage != MC_STORE_F16) return MC_ERR_UNSUPPORTED;
  XcGeom g;
  int rc = geom_from(q, &g, true, false);
  if (rc) return rc;
  if (!src || !job_off || !expo_a || !mask || !T1a || !tw_row || njobs < 1 || (expo_b && !T1b))
    return MC_ERR_ARG;
  if (!wave512_shape(g, mask)) return MC_ERR_UNSUPPORTED;
  return k1_wave512_launch(storage, src, job_off, row_stride, expo_a, expo_b, mask, mean_rstd, T1a, T1b, tw_row, njobs,
                           g, row_chord, nullptr, 1, nullptr, stream);
}

// N2: patch rows straight from the raw bytes of a u8 / i16 movie (the wave-per-row 1024-sample engine only).
int mc_xc_rows_forward_dual_raw(const void* raw, int storage, const float* gain, int64_t frame_area,
                                const int64_t* job_off, int64_t row_stride, const int* expo_a, const int* expo_b,
                                const float* mask, const float* job_sub, const float* mean_rstd, void* T1a, void* T1b,
                                const void* tw_row, int njobs, const mc_xc_geom* q, const int* row_chord,
                                void* stream) {
  if (storage != MC_STORE_U8 && storage != MC_STORE_I16) return MC_ERR_UNSUPPORTED;
  XcGeom g;
  int rc = geom_from(q, &g, true, false);
  if (rc) return rc;
  if (!raw || !gain || !job_off || !expo_a || !mask || !job_sub || !mean_rstd || !T1a || !tw_row || njobs < 1 ||
      (expo_b && !T1b) || frame_area < 1 || row_stride < 1)
    return MC_ERR_ARG;
  if (!wave512_shape(g, mask) || (reinterpret_cast<uintptr_t>(gain) & 3) ||
      (storage == MC_STORE_I16 && (reinterpret_cast<uintptr_t>(raw) & 1)))
    return MC_ERR_UNSUPPORTED;
  return k1_wave512_launch(storage, raw, job_off, row_stride, expo_a, expo_b, mask, mean_rstd, T1a, T1b, tw_row, njobs,
                           g, row_chord, gain, frame_area, job_sub, stream);
}

int mc_xc_rows_forward(const float* src, const int64_t* job_off, int64_t row_stride,
                       const int* job_expo, const float* mask, const float* mean_rstd,
                       void* T1, const void* tw_row, int njobs, const mc_xc_geom* q,
                       void* stream) {
  return rows_forward_impl(src, job_off, row_stride, job_expo, mask, mean_rstd, T1, tw_row, njobs, q,
                           nullptr, nullptr, stream);
}

int mc_xc_provisional_mean_t(const void* x, int storage, int n, float* m0, void* stream) {
  if (!x || !m0 || n < 1) return MC_ERR_ARG;
  if (storage != MC_STORE_F32 && storage != MC_STORE_F16) return MC_ERR_UNSUPPORTED;
  if (storage == MC_STORE_F32)
    hipLaunchKernelGGL(xc_provisional_mean_kernel<float>, dim3(1), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const float*>(x), n, m0);
  else
    hipLaunchKernelGGL(xc_provisional_mean_kernel<_Float16>, dim3(1), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const _Float16*>(x), n, m0);
  return mc_check_launch();
}

int mc_xc_rows_forward_stats_t(const void* src_any, int storage, const int64_t* job_off, int64_t row_stride,
                               const float* mask, const float* m0, void* T1, const void* tw_row,
                               int njobs, const mc_xc_geom* q, int hl, int hu, int wl, int wu,
                               double* acc, float* fix, float* out3, const int* row_chord, void* stream) {
  if (storage != MC_STORE_F32 && storage != MC_STORE_F16) return MC_ERR_UNSUPPORTED;
  const float* src = static_cast<const float*>(src_any);
  const bool half = storage == MC_STORE_F16;
  if (!m0 || !acc || !fix || !out3 || !q) return MC_ERR_ARG;
  if (hl < q->y0 || hu > q->y0 + q->ny || wl < q->x0 || wu > q->x1 || (wl & 1) || (wu & 1) ||
      hl >= hu || wl >= wu)
    return MC_ERR_ARG;  // the box must lie inside the region K1 reads
  hipError_t e = hipMemsetAsync(acc, 0, 2 * XC_STAT_SLOTS * sizeof(double), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  XcBox box{hl, hu, wl, wu};
  int rc = rows_forward_impl(src, job_off, row_stride, nullptr, mask, m0, T1, tw_row, njobs, q, &box,
                             acc, stream, row_chord, half);
  if (rc) return rc;
  const double count = (double)njobs * (hu - hl) * (wu - wl);
  hipLaunchKernelGGL(xc_stats_finalize, dim3(1), dim3(1), 0, (hipStream_t)stream, acc, count, m0, fix,
                     out3);
  return mc_check_launch();
}

// N2: K1 straight from the raw bytes of a u8 / i16 movie: A = (raw * gain - sub[job]) * mean_rstd[1] * mask.
// Whole-frame jobs: 4096-column frames on the wave-per-row engine, any other power-of-two width on the
// workgroup engine (mc_xcg_rows_forward_raw has the K3 formats); anything else is MC_ERR_UNSUPPORTED and the
// caller conditions the movie into an fp32 copy first (mc_condition_movie).
int mc_xc_rows_forward_raw(const void* raw, int storage, const float* gain, const int64_t* job_off,
                           int64_t row_stride, const float* mask, const float* job_sub, const float* mean_rstd,
                           void* T1, const void* tw_row, int njobs, const mc_xc_geom* q, const int* row_chord,
                           void* stream) {
  if (storage != MC_STORE_U8 && storage != MC_STORE_I16) return MC_ERR_UNSUPPORTED;
  XcGeom g;
  int rc = geom_from(q, &g, true, false);
  if (rc) return rc;
  if (!raw || !gain || !job_off || !mask || !job_sub || !mean_rstd || !T1 || !tw_row || njobs < 1) return MC_ERR_ARG;
  const int kind = storage == MC_STORE_U8 ? 1 : 2;
  const XcBox b{0, 0, 0, 0};
  if (k1_route(g, kind, false, raw, gain, mask, nullptr, row_stride, b, false) == K1_WG)
    // any other power-of-two width: the workgroup-per-row engine, element-wise loads of raw and gain
    return k1_wg_launch(kind, raw, job_off, row_stride, nullptr, mask, mean_rstd, T1, tw_row, njobs, g, b, nullptr, gain,
                        job_sub, stream);
  return k1_wave_launch(k1_wave_variant(g, kind, false, row_chord), kind, raw, job_off, row_stride, mask, mean_rstd, T1,
                        tw_row, njobs, g, b, nullptr, row_chord, gain, job_sub, stream);
}

// the sparse hot-pixel correction of T1 after mc_xc_rows_forward_raw (xc_rows_hot_fix)
int mc_xc_rows_hot_correct(const long long* keys, const float* rv, int64_t n, int frame0, int njobs, int h, int w,
                           const float* mask, const float* mean_rstd, void* T1, const mc_xc_geom* q, void* stream) {
  if (!keys || !rv || !mean_rstd || !T1 || !q || n < 0 || frame0 < 0 || njobs < 1 || h < 1 || w < 1 || q->W != w ||
      q->nkx < 1 || q->ny < 1 || q->y0 < 0 || q->y0 + q->ny > h || n > 0x7fffffffLL)
    return MC_ERR_ARG;
  if (n == 0) return MC_OK;
  hipLaunchKernelGGL(xc_rows_hot_fix, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, keys, (const float2*)rv, n,
                     frame0, njobs, h, w, mask, mean_rstd, (cfloat*)T1, q->W, q->nkx, q->y0, q->ny);
  return mc_check_launch();
}

}  // extern "C"
