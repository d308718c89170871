// Plan tables, filled once per plan: the circle mask and the band-pass / B-factor filter of the
// cross-correlation estimate; and mc_abi_version, which has no better home.
// All arithmetic that decides *which* pixels/bins are inside follows the fp32 op order of the torch
// expressions the reference evaluates, without FMA contraction.
#include "mc_common.h"
#include "mcorr.h"
#pragma clang fp contract(off)

// ------------------------------------------------------------------ circle mask
// torch_grid_utils.circle (xc.py:69-74): inside <=> sqrt(dy^2+dx^2) < radius in fp32.
__device__ __forceinline__ bool disk_inside(int dy, int dx, float radius) {
  const float fy = (float)dy, fx = (float)dx;
  return sqrtf(fy * fy + fx * fx) < radius;
}

// halfw[y] = largest a >= 0 with (y, cx +- a) inside, or -1 when the row is empty.
__global__ void mask_halfwidth(int* __restrict__ halfw, int h, int w, float radius) {
  const int y = blockIdx.x * blockDim.x + threadIdx.x;
  if (y >= h) return;
  const int cy = h / 2;
  int a = -1;
  for (int dx = 0; dx <= w; ++dx) {
    if (disk_inside(y - cy, dx, radius)) a = dx;
    else break;
  }
  halfw[y] = a;
}

__global__ void mask_fill(float* __restrict__ mask, const int* __restrict__ halfw, int h, int w,
                          float radius, float smoothing) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= w) return;
  const int cy = h / 2, cx = w / 2;
  const int dy = y - cy, dx = x - cx;
  float out = 0.f;
  if (disk_inside(dy, dx, radius)) {
    out = 1.f;
  } else if (smoothing > 0.f) {
    const double D = sqrt((double)dy * dy + (double)dx * dx);
    const double excess = D - (double)radius;
    if (excess <= (double)smoothing + 2.0) {
      // exact EDT to the digital disk: the nearest disk pixel is within excess+2 rows
      const int reach = (int)excess + 3;
      int lo = y - reach, hi = y + reach;
      if (lo < 0) lo = 0;
      if (hi > h - 1) hi = h - 1;
      long long best = -1;
      const int adx = dx < 0 ? -dx : dx;
      for (int yy = lo; yy <= hi; ++yy) {
        const int a = halfw[yy];
        if (a < 0) continue;
        // columns of the row that are inside and inside the image
        int gap;
        if (dx >= 0) {
          int right = cx + a;
          if (right > w - 1) right = w - 1;
          gap = x - right;
        } else {
          int left = cx - a;
          if (left < 0) left = 0;
          gap = left - x;
        }
        (void)adx;
        if (gap < 0) gap = 0;
        const long long ddy = (long long)(y - yy);
        const long long d2 = ddy * ddy + (long long)gap * gap;
        if (best < 0 || d2 < best) best = d2;
      }
      if (best > 0) {
        const float d = (float)sqrt((double)best);
        if (d <= smoothing) {
          const float halfpi = 1.5707963267948966f;
          out = cosf(halfpi * (d / smoothing));
        }
      }
    }
  }
  mask[(int64_t)y * w + x] = out;
}

// ------------------------------------------------------------------ xc filter
// torch.fft.fftfreq / rfftfreq: k * (1/n); norm = sqrt(fy^2 + fx^2) in fp32.
__global__ void xc_filter_fill(float* __restrict__ filt, int W, int H, int nkx, int kyp, int kyn,
                               float low, float high, float B, float pixel_size) {
  const int nky = kyp + kyn;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nkx * nky) return;
  const int kx = i / nky, kyi = i - kx * nky;
  const int ky = kyi < kyp ? kyi : kyi - kyp + (H - kyn);
  const int kk = (ky < (H + 1) / 2) ? ky : ky - H;
  const float fy = (float)kk * (float)(1.0 / (double)H);
  const float fx = (float)kx * (float)(1.0 / (double)W);
  const float f = sqrtf(fy * fy + fx * fx);
  float v = 0.f;
  if (f > low && f <= high) {
    const float fp = f / pixel_size;
    v = expf(-(B * (fp * fp)) / 4.f);
  }
  filt[i] = v;
}

extern "C" {

int mc_abi_version(void) { return MCORR_ABI_VERSION; }

int mc_circle_mask(float* mask, int* halfw, int h, int w, float radius, float smoothing_radius,
                   void* stream) {
  if (!mask || !halfw || h < 1 || w < 1 || !(radius >= 0.f) || !(smoothing_radius >= 0.f))
    return MC_ERR_ARG;
  hipLaunchKernelGGL(mask_halfwidth, dim3((h + 63) / 64), dim3(64), 0, (hipStream_t)stream, halfw,
                     h, w, radius);
  hipLaunchKernelGGL(mask_fill, dim3((w + 255) / 256, h), dim3(256), 0, (hipStream_t)stream, mask,
                     halfw, h, w, radius, smoothing_radius);
  return mc_check_launch();
}

int mc_xc_filter(float* filt, const mc_xc_geom* q, float low, float high, float b_factor,
                 float pixel_size, void* stream) {
  if (!filt || !q || q->nkx < 1 || q->kyp + q->kyn < 1 || !(pixel_size > 0.f)) return MC_ERR_ARG;
  const int n = q->nkx * (q->kyp + q->kyn);
  hipLaunchKernelGGL(xc_filter_fill, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     filt, q->W, q->H, q->nkx, q->kyp, q->kyn, low, high, b_factor, pixel_size);
  return mc_check_launch();
}

}  // extern "C"
