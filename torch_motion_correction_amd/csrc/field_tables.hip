// The lattice side of the deformation-field warp: the per-axis tap tables and the x-upsampled lattice E
// that every field-warp kernel reads (mc_field_tables_launch), the pixel-shift readers of those tables
// (mc_pixel_shifts, mc_pixel_shifts_at), and the cubic-spline evaluators that produce a lattice from a
// field in the first place (mc_spline_lattice, mc_spline_points).
//
// No FMA contraction in this object: warp_field_common.h says why.
#include "warp_field_common.h"
#pragma clang fp contract(off)

// ------------------------------------------------------------------ lattice tables and their readers
__device__ __forceinline__ int reflect_index(int i, int size) {
  const int span = size - 1;
  if (span <= 0) return 0;
  int a = i < 0 ? -i : i;
  const int flips = a / span;
  const int extra = a - flips * span;
  int r = (flips & 1) ? span - extra : extra;
  if (r < 0) r = 0;
  if (r > size - 1) r = size - 1;
  return r;
}

// Per-axis tables of the lattice upsample (get_pixel_shifts, correct_motion.py:161-179):
// for pixel index p of an axis of length n sampled from a lattice axis of length G.
__global__ void warp_axis_tables(int n, int G, int* __restrict__ tap, float* __restrict__ coef) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const float normalized = (float)p / (float)(n - 1);
  const float interp = normalized * (float)(G - 1);
  const float u = grid_chain(interp, (float)G);
  const float fl = floorf(u);
  float c[4];
  cubic_coeffs(u - fl, c);
  const int i0 = (int)fl;
  for (int k = 0; k < 4; ++k) {
    tap[4 * p + k] = reflect_index(i0 - 1 + k, G);
    coef[4 * p + k] = c[k];
  }
}

// E[f][c][R][x] = sum_j cx_j(x) * lattice[f][c][R][tap_j(x)]   (x-direction first)
__global__ void warp_etab(const float* __restrict__ lattice, int GH, int GW, int w,
                          const int* __restrict__ xtap, const float* __restrict__ xcoef,
                          float* __restrict__ etab) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int row = blockIdx.y;  // (f*2 + c)*GH + R
  if (x >= w) return;
  const float* L = lattice + (int64_t)row * GW;
  const int4 t = *reinterpret_cast<const int4*>(xtap + 4 * x);
  const float4 c = *reinterpret_cast<const float4*>(xcoef + 4 * x);
  etab[(int64_t)row * w + x] = ((c.x * L[t.x] + c.y * L[t.y]) + c.z * L[t.z]) + c.w * L[t.w];
}

// get_pixel_shifts (correct_motion.py:132-185) for one lattice: out (h, w, 2) px.
__global__ void warp_pixel_shifts(const float* __restrict__ etab, const int* __restrict__ ytap,
                                  const float* __restrict__ ycoef, int h, int w, int GH,
                                  float pixel_spacing, float* __restrict__ out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= w) return;
  const int4 yt = *reinterpret_cast<const int4*>(ytap + 4 * y);
  const float4 yc = *reinterpret_cast<const float4*>(ycoef + 4 * y);
  for (int c = 0; c < 2; ++c) {
    const float* E = etab + (int64_t)c * GH * w + x;
    const float s = ((yc.x * E[(int64_t)yt.x * w] + yc.y * E[(int64_t)yt.y * w]) +
                     yc.z * E[(int64_t)yt.z * w]) + yc.w * E[(int64_t)yt.w * w];
    out[((int64_t)y * w + x) * 2 + c] = s / pixel_spacing;
  }
}

// get_pixel_shifts at caller-supplied pixel coordinates (the `pixel_grid` argument,
// correct_motion.py:167-168): coords (n, 2) yx in pixels of an (h, w) frame -> out (n, 2) px.
// Same fp32 chain as warp_axis_tables with (float)p replaced by the given coordinate; x taps
// first, then y (ATen's bicubic grid_sample order), reflection padding per tap.
__global__ void warp_pixel_shifts_at(const float* __restrict__ lattice, int GH, int GW, int h, int w,
                                     float pixel_spacing, const float* __restrict__ coords, int64_t n,
                                     float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int tap[2][4];
  float coef[2][4];
  for (int axis = 0; axis < 2; ++axis) {
    const int len = axis == 0 ? h : w, G = axis == 0 ? GH : GW;
    const float normalized = coords[2 * i + axis] / (float)(len - 1);
    const float interp = normalized * (float)(G - 1);
    const float u = grid_chain(interp, (float)G);
    const float fl = floorf(u);
    cubic_coeffs(u - fl, coef[axis]);
    // clamp in float first: a far-away coordinate must not overflow the int conversion
    const int i0 = (int)fminf(fmaxf(fl, -1.0e9f), 1.0e9f);
    for (int k = 0; k < 4; ++k) tap[axis][k] = reflect_index(i0 - 1 + k, G);
  }
  for (int c = 0; c < 2; ++c) {
    const float* L = lattice + (int64_t)c * GH * GW;
    float rowv[4];
    for (int ky = 0; ky < 4; ++ky) {
      const float* r = L + (int64_t)tap[0][ky] * GW;
      rowv[ky] = ((coef[1][0] * r[tap[1][0]] + coef[1][1] * r[tap[1][1]]) + coef[1][2] * r[tap[1][2]]) +
                 coef[1][3] * r[tap[1][3]];
    }
    const float sft = ((coef[0][0] * rowv[0] + coef[0][1] * rowv[1]) + coef[0][2] * rowv[2]) + coef[0][3] * rowv[3];
    out[2 * i + c] = sft / pixel_spacing;
  }
}

// ------------------------------------------------------------------ spline lattice
// out[c][it][iy][ix] = sum_kt wt sum_ky wy sum_kx wx * data[c][idx_t][idx_y][idx_x]
// (x innermost, then y, then t -- the separable order of the spline library).
__global__ void spline_lattice_kernel(const float* __restrict__ data, int c, int nt, int nh, int nw,
                                      const int* __restrict__ idx_t, const float* __restrict__ w_t,
                                      int NT, const int* __restrict__ idx_y,
                                      const float* __restrict__ w_y, int NY,
                                      const int* __restrict__ idx_x, const float* __restrict__ w_x,
                                      int NX, float* __restrict__ out) {
  const int64_t total = (int64_t)c * NT * NY * NX;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int ix = (int)(i % NX);
  const int iy = (int)((i / NX) % NY);
  const int it = (int)((i / ((int64_t)NX * NY)) % NT);
  const int ch = (int)(i / ((int64_t)NX * NY * NT));
  const float* d = data + (int64_t)ch * nt * nh * nw;
  float vt = 0.f;
  for (int kt = 0; kt < 4; ++kt) {
    const float* dt = d + (int64_t)idx_t[4 * it + kt] * nh * nw;
    float vy = 0.f;
    for (int ky = 0; ky < 4; ++ky) {
      const float* dy = dt + (int64_t)idx_y[4 * iy + ky] * nw;
      float vx = 0.f;
      for (int kx = 0; kx < 4; ++kx) vx += dy[idx_x[4 * ix + kx]] * w_x[4 * ix + kx];
      vy += vx * w_y[4 * iy + ky];
    }
    vt += vy * w_t[4 * it + kt];
  }
  out[i] = vt;
}

// Spline grid at scattered points: per point 3 x 4 taps (host tables, as for the lattice); same
// summation order as spline_lattice_kernel.  out[i][ch].
__global__ void spline_points_kernel(const float* __restrict__ data, int c, int nt, int nh, int nw,
                                     const int* __restrict__ idx_t, const float* __restrict__ w_t,
                                     const int* __restrict__ idx_y, const float* __restrict__ w_y,
                                     const int* __restrict__ idx_x, const float* __restrict__ w_x,
                                     int64_t npoints, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npoints * c) return;
  const int64_t pt = i / c;
  const int ch = (int)(i - pt * c);
  const float* d = data + (int64_t)ch * nt * nh * nw;
  float vt = 0.f;
  for (int kt = 0; kt < 4; ++kt) {
    const float* dt = d + (int64_t)idx_t[4 * pt + kt] * nh * nw;
    float vy = 0.f;
    for (int ky = 0; ky < 4; ++ky) {
      const float* dy = dt + (int64_t)idx_y[4 * pt + ky] * nw;
      float vx = 0.f;
      for (int kx = 0; kx < 4; ++kx) vx += dy[idx_x[4 * pt + kx]] * w_x[4 * pt + kx];
      vy += vx * w_y[4 * pt + ky];
    }
    vt += vy * w_t[4 * pt + kt];
  }
  out[i] = vt;
}

// ------------------------------------------------------------------ host side
// the per-axis tap tables and the x-upsampled lattice E of `nframes` lattices (declared in warp_field_common.h)
void mc_field_tables_launch(const float* lattice, int nframes, int h, int w, int GH, int GW, const FieldScratch& t,
                            hipStream_t s) {
  hipLaunchKernelGGL(warp_axis_tables, dim3((h + 255) / 256), dim3(256), 0, s, h, GH, t.ytap, t.ycoef);
  hipLaunchKernelGGL(warp_axis_tables, dim3((w + 255) / 256), dim3(256), 0, s, w, GW, t.xtap, t.xcoef);
  hipLaunchKernelGGL(warp_etab, dim3((w + 255) / 256, nframes * 2 * GH), dim3(256), 0, s, lattice, GH, GW, w,
                     (const int*)t.xtap, (const float*)t.xcoef, t.etab);
}

extern "C" {

int mc_spline_lattice(const float* data, int c, int nt, int nh, int nw, const int* idx_t,
                      const float* w_t, int NT, const int* idx_y, const float* w_y, int NY,
                      const int* idx_x, const float* w_x, int NX, float* out, void* stream) {
  if (!data || !idx_t || !w_t || !idx_y || !w_y || !idx_x || !w_x || !out) return MC_ERR_ARG;
  if (c < 1 || nt < 1 || nh < 1 || nw < 1 || NT < 1 || NY < 1 || NX < 1) return MC_ERR_ARG;
  const int64_t total = (int64_t)c * NT * NY * NX;
  hipLaunchKernelGGL(spline_lattice_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, data, c, nt, nh, nw, idx_t, w_t, NT, idx_y, w_y, NY,
                     idx_x, w_x, NX, out);
  return mc_check_launch();
}

int mc_spline_points(const float* data, int c, int nt, int nh, int nw, const int* idx_t, const float* w_t,
                     const int* idx_y, const float* w_y, const int* idx_x, const float* w_x, int64_t npoints,
                     float* out, void* stream) {
  if (!data || !idx_t || !w_t || !idx_y || !w_y || !idx_x || !w_x || !out) return MC_ERR_ARG;
  if (c < 1 || nt < 1 || nh < 1 || nw < 1 || npoints < 1) return MC_ERR_ARG;
  const int64_t total = npoints * c;
  hipLaunchKernelGGL(spline_points_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, data, c, nt, nh, nw, idx_t, w_t, idx_y, w_y, idx_x, w_x, npoints, out);
  return mc_check_launch();
}

int mc_warp_scratch_bytes(int nframes, int h, int w, int GH, int GW, int64_t* bytes) {
  if (!bytes || nframes < 1 || h < 2 || w < 2 || GH < 1 || GW < 1) return MC_ERR_ARG;
  *bytes = field_scratch(nullptr, nframes, h, w, GH).bytes;
  return MC_OK;
}

int mc_pixel_shifts(const float* lattice, int GH, int GW, int h, int w, float pixel_spacing,
                    float* scratch, float* out, void* stream) {
  if (!lattice || !scratch || !out || h < 2 || w < 2 || GH < 1 || GW < 1 || !(pixel_spacing > 0.f))
    return MC_ERR_ARG;
  if (((uintptr_t)scratch) & 15) return MC_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const FieldScratch t = field_scratch(scratch, 1, h, w, GH);
  mc_field_tables_launch(lattice, 1, h, w, GH, GW, t, s);
  hipLaunchKernelGGL(warp_pixel_shifts, dim3((w + 255) / 256, h), dim3(256), 0, s, (const float*)t.etab,
                     (const int*)t.ytap, (const float*)t.ycoef, h, w, GH, pixel_spacing, out);
  return mc_check_launch();
}

int mc_pixel_shifts_at(const float* lattice, int GH, int GW, int h, int w, float pixel_spacing,
                       const float* coords_yx, int64_t n, float* out, void* stream) {
  if (!lattice || !coords_yx || !out || h < 2 || w < 2 || GH < 1 || GW < 1 || n < 1 || !(pixel_spacing > 0.f))
    return MC_ERR_ARG;
  hipLaunchKernelGGL(warp_pixel_shifts_at, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, lattice, GH, GW, h, w, pixel_spacing, coords_yx, n, out);
  return mc_check_launch();
}

}  // extern "C"
