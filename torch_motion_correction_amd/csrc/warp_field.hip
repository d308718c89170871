// Deformation-field warp: cubic-spline lattice evaluation, bicubic shift upsample and
// bicubic frame resample (+ optional fused frame sum).
//
// Reference path (correct_motion.py:18-185, deformation_field_utils.py:9-93): per frame
//   lattice(2,10gh,10gw) = spline(field)(t_i, linspace, linspace)
//   shifts(h,w,2)        = grid_sample(lattice, bicubic, reflection, align_corners) / pixel_spacing
//   out(h,w)             = grid_sample(frame, pixel+shift, bicubic, border, align_corners),
//                          zero where the coordinate leaves [0,h-1]x[0,w-1]
// The reference materialises the coordinate grid, the normalised grid and the shift
// grid (3 x 128 MiB per 4096^2 frame) and gathers 16+16 taps per pixel.  Here the
// x-direction of the shift upsample is hoisted into a small per-frame table
// E[c][lattice row][x] (the reference's own summation order: x taps first, then y),
// so each pixel needs 4 table rows per channel; coordinates live in registers only.
//
// The fp32 coordinate chain is reproduced operation by operation: at coordinates ~4096 one ulp is
// 2.4e-4 px, which is visible at the 1e-4 parity bar.  So this file's mode is NO FMA contraction; the
// few helpers that form resampling weights and tap sums may contract and say so in their own bodies.
#include "warp_common.h"
#include "mcorr.h"
#pragma clang fp contract(off)

// Measured settings (DESIGN.md section 4 has the alternatives)
#define GW2_MINW 3  // warp_field2: workgroups per CU the register budget is held to
#define GW3_ILP 1   // warp_field3: pixels of a lane in flight together (interior tile-frames); 1, 2 and 4 measure the same

// s / d for a loop-invariant divisor, same three-instruction correctly rounded form
__device__ __forceinline__ float div_invariant(float s, float d) {
  const float r = 1.0f / d;
  const float q = s * r;
  return __builtin_fmaf(__builtin_fmaf(-q, d, s), r, q);
}

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

#define WARP_TX 32   // threads across, 4 px each -> 128 px
#define WARP_TY 8    // thread rows, 2 adjacent pixel rows each -> 16 rows
#define WARP_PX 4
#define WARP_ROWS 2

struct WarpArgs {
  const float* frames;
  int nframes, h, w, GH;
  const float* etab;   // [f][2][GH][w]
  const int* ytap;     // [h][4]
  const float* ycoef;  // [h][4]
  float pixel_spacing;
  float* out_frames;
  float* out_sum;
  int tiles_x, tiles_y;
};

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));  // dword-aligned 16-B load


// What is not the coordinate chain may contract to FMA (see cubic_coeffs_fast)
__device__ __forceinline__ float dot4(const float4 c, float e0, float e1, float e2, float e3) {
#pragma clang fp contract(fast)
  return ((c.x * e0 + c.y * e1) + c.z * e2) + c.w * e3;
}
// 5-tap accumulate: taps 0..4 of a window, weights shifted by one when `up`
__device__ __forceinline__ float dot5(const float wt[4], bool up, float v0, float v1, float v2,
                                      float v3, float v4) {
#pragma clang fp contract(fast)
  const float a0 = up ? 0.f : wt[0];
  const float a1 = up ? wt[0] : wt[1];
  const float a2 = up ? wt[1] : wt[2];
  const float a3 = up ? wt[2] : wt[3];
  const float a4 = up ? wt[3] : 0.f;
  return (((a0 * v0 + a1 * v1) + a2 * v2) + a3 * v3) + a4 * v4;
}

struct TapWindow {   // rows by..by+4, cols bx..bx+7 of one frame
  float v[5][8];
  int by, bx;
  bool valid;
};

__device__ __forceinline__ void window_load_row(TapWindow& win, int i, const float* fr, int w) {
  const float* r = fr + (int64_t)(win.by + i) * w + win.bx;
  const f4u lo = *reinterpret_cast<const f4u*>(r);
  const f4u hi = *reinterpret_cast<const f4u*>(r + 4);
  win.v[i][0] = lo.x; win.v[i][1] = lo.y; win.v[i][2] = lo.z; win.v[i][3] = lo.w;
  win.v[i][4] = hi.x; win.v[i][5] = hi.y; win.v[i][6] = hi.z; win.v[i][7] = hi.w;
}

// Position the window at (by, bx); reuse rows when it only moved down by one.
__device__ __forceinline__ void window_seek(TapWindow& win, int by, int bx, const float* fr, int w) {
  if (win.valid && win.bx == bx && win.by == by) return;
  if (win.valid && win.bx == bx && win.by + 1 == by) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) win.v[i][j] = win.v[i + 1][j];
    win.by = by;
    window_load_row(win, 4, fr, w);
    return;
  }
  win.by = by;
  win.bx = bx;
  win.valid = true;
#pragma unroll
  for (int i = 0; i < 5; ++i) window_load_row(win, i, fr, w);
}

template <bool UNIT_PS>
__device__ __forceinline__ void warp_row(const WarpArgs& a, const float* fr, int y, int x0,
                                         const float4 yc, const float4 Ey[4], const float4 Ex[4],
                                         TapWindow& win, float res[WARP_PX]) {
  const int h = a.h, w = a.w;
  const float fh = (float)h, fw = (float)w;
  float uy[WARP_PX], ux[WARP_PX], fy[WARP_PX], fx[WARP_PX];
  bool inside[WARP_PX];
  const float ey[4][4] = {{Ey[0].x, Ey[0].y, Ey[0].z, Ey[0].w}, {Ey[1].x, Ey[1].y, Ey[1].z, Ey[1].w},
                          {Ey[2].x, Ey[2].y, Ey[2].z, Ey[2].w}, {Ey[3].x, Ey[3].y, Ey[3].z, Ey[3].w}};
  const float ex[4][4] = {{Ex[0].x, Ex[0].y, Ex[0].z, Ex[0].w}, {Ex[1].x, Ex[1].y, Ex[1].z, Ex[1].w},
                          {Ex[2].x, Ex[2].y, Ex[2].z, Ex[2].w}, {Ex[3].x, Ex[3].y, Ex[3].z, Ex[3].w}};
  float fby = 3.0e38f, fbx = 3.0e38f;
#pragma unroll
  for (int k = 0; k < WARP_PX; ++k) {
    float sy = dot4(yc, ey[0][k], ey[1][k], ey[2][k], ey[3][k]);
    float sx = dot4(yc, ex[0][k], ex[1][k], ex[2][k], ex[3][k]);
    if (!UNIT_PS) {
      sy = div_invariant(sy, a.pixel_spacing);
      sx = div_invariant(sx, a.pixel_spacing);
    }
    const float cy = (float)y + sy, cx = (float)(x0 + k) + sx;
    inside[k] = (cy >= 0.f) && (cy <= fh - 1.f) && (cx >= 0.f) && (cx <= fw - 1.f);
    uy[k] = grid_chain(cy, fh);
    ux[k] = grid_chain(cx, fw);
    fy[k] = floorf(uy[k]);
    fx[k] = floorf(ux[k]);
    fby = fminf(fby, fy[k]);
    fbx = fminf(fbx, fx[k] - (float)k);
  }
  bool ok = (fby >= 1.f) && (fby + 3.f <= fh - 1.f) && (fbx >= 1.f) && (fbx + 6.f <= fw - 1.f);
#pragma unroll
  for (int k = 0; k < WARP_PX; ++k) {
    const float dy = fy[k] - fby, dx = fx[k] - (float)k - fbx;
    ok = ok && (dy == 0.f || dy == 1.f) && (dx == 0.f || dx == 1.f);
  }
  if (ok) {
    window_seek(win, (int)fby - 1, (int)fbx - 1, fr, w);
#pragma unroll
    for (int k = 0; k < WARP_PX; ++k) {
      float wy[4], wx[4];
      cubic_coeffs_fast(uy[k] - fy[k], wy);
      cubic_coeffs_fast(ux[k] - fx[k], wx);
      const bool upy = fy[k] != fby, upx = (fx[k] - (float)k) != fbx;
      float rowv[5];
#pragma unroll
      for (int i = 0; i < 5; ++i)
        rowv[i] = dot5(wx, upx, win.v[i][k], win.v[i][k + 1], win.v[i][k + 2], win.v[i][k + 3],
                       win.v[i][k + 4]);
      const float o = dot5(wy, upy, rowv[0], rowv[1], rowv[2], rowv[3], rowv[4]);
      res[k] = inside[k] ? o : 0.f;
    }
  } else {
#pragma unroll
    for (int k = 0; k < WARP_PX; ++k) {
      float wy[4], wx[4];
      cubic_coeffs_fast(uy[k] - fy[k], wy);
      cubic_coeffs_fast(ux[k] - fx[k], wx);
      // border padding: clip each tap coordinate (ATen clip_coordinates), in float first
      // so that huge coordinates cannot overflow the int conversion
      float rowv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float ty = fminf(fmaxf(fy[k] + (float)(i - 1), 0.f), fh - 1.f);
        const float* r = fr + (int64_t)(int)ty * w;
        float t4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          t4[j] = r[(int)fminf(fmaxf(fx[k] + (float)(j - 1), 0.f), fw - 1.f)];
        rowv[i] = dot4(make_float4(wx[0], wx[1], wx[2], wx[3]), t4[0], t4[1], t4[2], t4[3]);
      }
      const float o = dot4(make_float4(wy[0], wy[1], wy[2], wy[3]), rowv[0], rowv[1], rowv[2], rowv[3]);
      res[k] = inside[k] ? o : 0.f;
    }
  }
}

__device__ __forceinline__ void load_etab4(const float* E, int64_t rowstride, const int4 yt, int x0,
                                           int w, float4 out[4]) {
  const int rows[4] = {yt.x, yt.y, yt.z, yt.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float* p = E + (int64_t)rows[i] * rowstride + x0;
    if (x0 + 3 < w && ((rowstride & 3) == 0)) {
      out[i] = *reinterpret_cast<const float4*>(p);
    } else {
      out[i].x = p[0];
      out[i].y = x0 + 1 < w ? p[1] : 0.f;
      out[i].z = x0 + 2 < w ? p[2] : 0.f;
      out[i].w = x0 + 3 < w ? p[3] : 0.f;
    }
  }
}

template <bool WRITE_FRAMES, bool WRITE_SUM, bool UNIT_PS>
__global__ __launch_bounds__(WARP_TX* WARP_TY) void warp_main(WarpArgs a) {
  // XCD-aware tile order: blocks b, b+8, b+16.. share an XCD (round-robin dispatch);
  // give each XCD a contiguous band of tile rows so vertical halos hit its own L2.
  const int nt = a.tiles_x * a.tiles_y;
  const int b = blockIdx.x;
  int tile = b;
  if ((nt & 7) == 0) tile = (b & 7) * (nt >> 3) + (b >> 3);
  const int tyi = tile / a.tiles_x, txi = tile - tyi * a.tiles_x;
  const int x0 = txi * (WARP_TX * WARP_PX) + threadIdx.x * WARP_PX;
  const int ya = tyi * (WARP_TY * WARP_ROWS) + threadIdx.y * WARP_ROWS;
  const int h = a.h, w = a.w;
  if (ya >= h || x0 >= w) return;
  const int64_t hw = (int64_t)h * w;
  const bool two = (ya + 1 < h);
  const int yb = two ? ya + 1 : ya;
  const int4 yta = *reinterpret_cast<const int4*>(a.ytap + 4 * ya);
  const float4 yca = *reinterpret_cast<const float4*>(a.ycoef + 4 * ya);
  const int4 ytb = *reinterpret_cast<const int4*>(a.ytap + 4 * yb);
  const float4 ycb = *reinterpret_cast<const float4*>(a.ycoef + 4 * yb);
  const bool same = (yta.x == ytb.x) && (yta.y == ytb.y) && (yta.z == ytb.z) && (yta.w == ytb.w);
  const bool full = (x0 + WARP_PX <= w);
  float acc[WARP_ROWS][WARP_PX] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};

  for (int f = 0; f < a.nframes; ++f) {
    const float* fr = a.frames + (int64_t)f * hw;
    const float* E = a.etab + (int64_t)f * 2 * a.GH * w;
    float4 Ey[4], Ex[4];
    load_etab4(E, w, yta, x0, w, Ey);
    load_etab4(E + (int64_t)a.GH * w, w, yta, x0, w, Ex);
    TapWindow win;
    win.valid = false;
    win.by = win.bx = 0;
    float res[WARP_ROWS][WARP_PX];
    warp_row<UNIT_PS>(a, fr, ya, x0, yca, Ey, Ex, win, res[0]);
    if (two) {
      if (!same) {
        load_etab4(E, w, ytb, x0, w, Ey);
        load_etab4(E + (int64_t)a.GH * w, w, ytb, x0, w, Ex);
      }
      warp_row<UNIT_PS>(a, fr, yb, x0, ycb, Ey, Ex, win, res[1]);
    }
#pragma unroll
    for (int r = 0; r < WARP_ROWS; ++r) {
      if (r == 1 && !two) break;
      if (WRITE_FRAMES) {
        float* o = a.out_frames + (int64_t)f * hw + (int64_t)(ya + r) * w + x0;
        if (full && ((((uintptr_t)o) & 15) == 0)) {
          *reinterpret_cast<float4*>(o) = make_float4(res[r][0], res[r][1], res[r][2], res[r][3]);
        } else {
          for (int k = 0; k < WARP_PX && x0 + k < w; ++k) o[k] = res[r][k];
        }
      }
      if (WRITE_SUM) {
#pragma unroll
        for (int k = 0; k < WARP_PX; ++k) acc[r][k] += res[r][k];
      }
    }
  }
  if (WRITE_SUM) {
    for (int r = 0; r < WARP_ROWS; ++r) {
      if (r == 1 && !two) break;
      float* o = a.out_sum + (int64_t)(ya + r) * w + x0;
      for (int k = 0; k < WARP_PX && x0 + k < w; ++k) o[k] = acc[r][k];  // this thread owns the pixel for all frames
    }
  }
}

// ------------------------------------------------------------------ general warp, LDS tile
// Per (tile, frame): the shift at the tile centre positions a (32+3+2*MG) x (256+3+2*MG)
// input window that is DMA'd into LDS; every pixel then runs the reference's per-pixel
// coordinate chain (strict fp32, see file header) and gathers its 4x4 taps from LDS.
// Lane l owns pixels x = x_tile + l + 64k (k = 0..3): adjacent lanes read adjacent LDS
// words, so the data-dependent gathers are bank-conflict free.
//
// Whether ALL taps of a tile fit the window is decided up front, rigorously: a pixel's
// shift is a bicubic (A = -0.75) interpolation of lattice nodes, sum(w) = 1 and
// sum|w| <= 1.375^2 < 1.9 in 2-D, so with rho = half the range of the nodes that can
// influence the tile every shift lies within 1.9*rho of the mid-range value and within
// 3.8*rho of the centre pixel's.  Tile-frames that fail the test are only flagged here and
// are processed afterwards by warp_field_slow (generic global gathers).
// The x-direction of the shift-lattice upsample comes from the E table (warp_etab); a
// thread caches its 4 px x 4 lattice rows x 2 channels of E in registers while
// consecutive pixel rows use the same lattice rows (they almost always do).
#define GW_MG 6
#define GW_ROWS (RIGID_WAVES * RIGID_ROWS + 3 + 2 * GW_MG)              // 47
#define GW_QUADS ((RIGID_LANES * 4 + 3 + 2 * GW_MG + 3 + 3) / 4)         // 70 (alignment slack)
#define GW_STRIDE (4 * GW_QUADS)                                          // 280 floats
#define GW_NQ (GW_ROWS * GW_QUADS)
#define GW_QUADS_PAD (((GW_NQ + 63) / 64) * 64)

__device__ __forceinline__ float gw_dot4(const float w[4], float a, float b, float c, float d) {
#pragma clang fp contract(fast)
  return ((w[0] * a + w[1] * b) + w[2] * c) + w[3] * d;
}

struct FieldArgs {
  WarpArgs w;
  const float* lattice;  // [f][2][GH][GW]
  const int* xtap;       // [w][4]
  int GW;
  unsigned char* flags;  // [f][tile]: 1 = irregular, left to warp_field_slow
  const float* gain;     // raw frames (N2) only: (h, w) gain reference
  const float* mu;       // raw frames (N2) only: [f] frame means, subtracted after the gain multiply
};

__device__ __forceinline__ int wave_min_i(int v) {
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ float wave_min_f(float v) {
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

// ------------------------------------------------------------------ general warp, second version
// Same tiling, window DMA and per-pixel chain as the first LDS-tile kernel (warp_field, since removed),
// rebuilt around what limits it -- VALU issue and the number of window bytes:
//  * the window margin follows the field: mg = ceil(3.8 rho + 1.05) per axis and tile-frame (2 for
//    the smooth fields of real movies) instead of the fixed 6, lanes outside the needed window
//    issue no DMA (window bytes 1.6x -> 1.3x of the tile);
//  * 3 workgroups per CU (one 52 KB window each), so a workgroup's DMA wait hides under two others;
//  * tile-frames whose window lies inside the image (all but the frame's rim) take a body without
//    the zero-outside test and without index clamps;
//  * cubic-convolution weights in factored form: c0 = A t u^2, c3 = A u t^2, c1 = 1 - t^2 ((A+3) -
//    (A+2) t), c2 likewise in u = 1 - t (11 instead of 17 operations per axis; the same polynomials
//    as ATen's Horner forms, values equal to ~1e-7).
__device__ __forceinline__ void cubic_coeffs_factored(float t, float c[4]) {
#pragma clang fp contract(fast)
  const float A = -0.75f;
  const float u = 1.f - t;
  const float atu = (A * t) * u;
  c[0] = atu * u;
  c[3] = atu * t;
  c[1] = 1.f - (t * t) * ((A + 3.f) - (A + 2.f) * t);
  c[2] = 1.f - (u * u) * ((A + 3.f) - (A + 2.f) * u);
}

template <bool WRITE_FRAMES, bool WRITE_SUM, bool UNIT_PS>
__global__ __launch_bounds__(RIGID_LANES* RIGID_WAVES, GW2_MINW) void warp_field2(FieldArgs fa) {
  const WarpArgs& a = fa.w;
  extern __shared__ __attribute__((aligned(16))) char smem_gw[];
  float4* const tile4 = reinterpret_cast<float4*>(smem_gw);
  float* const tile = reinterpret_cast<float*>(smem_gw);
  __shared__ int s_ytap[RIGID_WAVES * RIGID_ROWS][4];
  __shared__ float s_ycoef[RIGID_WAVES * RIGID_ROWS][4];
  const int nt = a.tiles_x * a.tiles_y;
  const int b = blockIdx.x;
  int tl = b;
  if ((nt & 7) == 0) tl = (b & 7) * (nt >> 3) + (b >> 3);
  const int tyi = tl / a.tiles_x, txi = tl - tyi * a.tiles_x;
  const int h = a.h, w = a.w;
  const float fh = (float)h, fw = (float)w;
  const int lane = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int tid = wave * RIGID_LANES + lane;
  const int xt = txi * (RIGID_LANES * 4);
  const int yt = tyi * (RIGID_WAVES * RIGID_ROWS);
  const int y0 = yt + wave * RIGID_ROWS;
  const int64_t hw = (int64_t)h * w;
  if (tid < RIGID_WAVES * RIGID_ROWS) {  // frame-invariant per-row lattice taps of this tile
    const int y = yt + tid < h ? yt + tid : h - 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s_ytap[tid][k] = a.ytap[4 * y + k];
      s_ycoef[tid][k] = a.ycoef[4 * y + k];
    }
  }
  // lattice footprint of the tile (frame-invariant): node rows [R0,R1], node columns [C0,C1]
  int R0, R1, C0, C1;
  {
    int lo = 0x7fffffff, hi = -1;
    if (lane < RIGID_WAVES * RIGID_ROWS) {
      const int y = yt + lane < h ? yt + lane : h - 1;
      for (int k = 0; k < 4; ++k) {
        const int v = a.ytap[4 * y + k];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
      }
    }
    R0 = wave_min_i(lo);
    R1 = wave_max_i(hi);
    lo = 0x7fffffff;
    hi = -1;
    for (int k = 0; k < 4; ++k) {
      const int x = xt + lane + 64 * k;
      const int xs = x < w ? x : w - 1;
      for (int j = 0; j < 4; ++j) {
        const int v = fa.xtap[4 * xs + j];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
      }
    }
    C0 = wave_min_i(lo);
    C1 = wave_max_i(hi);
  }
  const int yc = (yt + 16 < h) ? yt + 16 : h - 1;  // centre pixel of the tile (clipped to the image)
  const int xc = (xt + 128 < w) ? xt + 128 : w - 1;
  const int4 ytc = *reinterpret_cast<const int4*>(a.ytap + 4 * yc);
  const float4 ycc = *reinterpret_cast<const float4*>(a.ycoef + 4 * yc);
  const bool whole_tile = yt + RIGID_WAVES * RIGID_ROWS <= h && xt + RIGID_LANES * 4 <= w;
  float acc[RIGID_ROWS][4];
#pragma unroll
  for (int r = 0; r < RIGID_ROWS; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[r][k] = 0.f;
  __syncthreads();

  for (int f = 0; f < a.nframes; ++f) {
    const float* fr = a.frames + (int64_t)f * hw;
    const float* E = a.etab + (int64_t)f * 2 * a.GH * w;
    const int64_t chs = (int64_t)a.GH * w;  // channel stride of E
    // 0. regularity -> window margins: range of the lattice nodes that can influence this tile.
    // |shift - shift_centre| <= 3.8 rho (bicubic: sum|w| < 1.9 in 2-D, twice for the centre's own
    // deviation); taps span [-1,+2] around floor(); coordinate rounding adds < 0.01 px.
    int mgy, mgx;
    {
      const float* L = fa.lattice + (int64_t)f * 2 * a.GH * fa.GW;
      const int ncol = C1 - C0 + 1, nnode = (R1 - R0 + 1) * ncol;
      float lo_y = 3.0e38f, hi_y = -3.0e38f, lo_x = 3.0e38f, hi_x = -3.0e38f;
      for (int i = lane; i < nnode; i += RIGID_LANES) {
        const int R = R0 + i / ncol, Cc = C0 + i % ncol;
        const float vy = L[(int64_t)R * fa.GW + Cc], vx = L[(int64_t)(a.GH + R) * fa.GW + Cc];
        lo_y = fminf(lo_y, vy); hi_y = fmaxf(hi_y, vy);
        lo_x = fminf(lo_x, vx); hi_x = fmaxf(hi_x, vx);
      }
      const float ry = 0.5f * (wave_max_f(hi_y) - wave_min_f(lo_y)) / a.pixel_spacing;
      const float rx = 0.5f * (wave_max_f(hi_x) - wave_min_f(lo_x)) / a.pixel_spacing;
      const float ny = 3.8f * ry + 1.05f, nx = 3.8f * rx + 1.05f;
      // NaNs fail the comparison and go to the slow kernel (workgroup-uniform: every wave
      // computed the same numbers)
      if (!((ny <= (float)GW_MG) && (nx <= (float)GW_MG))) {
        if (tid == 0) fa.flags[(int64_t)f * nt + tl] = 1;
        continue;
      }
      mgy = __builtin_amdgcn_readfirstlane((int)ceilf(ny));
      mgx = __builtin_amdgcn_readfirstlane((int)ceilf(nx));
    }
    const int nrows = RIGID_WAVES * RIGID_ROWS + 3 + 2 * mgy;          // <= GW_ROWS
    int nq = (RIGID_LANES * 4 + 6 + 2 * mgx + 3) / 4;                    // <= GW_QUADS
    nq = nq < GW_QUADS ? nq : GW_QUADS;
    // 1. window origin from the shift at the tile centre (identical in every lane)
    int wy0, ax;
    {
      const float* Ec = E + xc;
      float sy = dot4(ycc, Ec[(int64_t)ytc.x * w], Ec[(int64_t)ytc.y * w], Ec[(int64_t)ytc.z * w],
                      Ec[(int64_t)ytc.w * w]);
      float sx = dot4(ycc, Ec[chs + (int64_t)ytc.x * w], Ec[chs + (int64_t)ytc.y * w],
                      Ec[chs + (int64_t)ytc.z * w], Ec[chs + (int64_t)ytc.w * w]);
      if (!UNIT_PS) {
        sy = div_invariant(sy, a.pixel_spacing);
        sx = div_invariant(sx, a.pixel_spacing);
      }
      const float lim = 4.f * (fh + fw);
      const float dy = fminf(fmaxf(floorf(grid_chain((float)yc + sy, fh)) - (float)yc, -lim), lim);
      const float dx = fminf(fmaxf(floorf(grid_chain((float)xc + sx, fw)) - (float)xc, -lim), lim);
      wy0 = __builtin_amdgcn_readfirstlane(yt + (int)dy - 1 - mgy);
      ax = __builtin_amdgcn_readfirstlane((xt + (int)dx - 1 - mgx) & ~3);
    }
    // 2. window -> LDS (the previous frame's reads are behind the barrier at the loop's end); the
    // LDS image keeps the fixed row stride, lanes outside the needed rows / quads issue nothing
    for (int i = wave; i < GW_QUADS_PAD / 64; i += RIGID_WAVES) {
      const int q = i * 64 + lane;
      const int tr = q / GW_QUADS, qc = q - tr * GW_QUADS;
      if (tr < nrows && qc < nq) {
        int r = wy0 + tr;
        r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
        int c = ax + 4 * qc;
        c = c < 0 ? 0 : (c > w - 4 ? w - 4 : c);
        __builtin_amdgcn_global_load_lds(fr + (int64_t)r * w + c, (lds_vptr)(tile4 + i * 64), 16, 0, 0);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool interior = whole_tile && wy0 >= 0 && wy0 + nrows <= h && ax >= 0 && ax + 4 * nq <= w;
    if (ax < 0 || ax + 4 * nq > w) {  // border padding: clipped columns (edge tiles only)
      for (int i = tid; i < nrows * GW_STRIDE; i += RIGID_LANES * RIGID_WAVES) {
        const int tr = i / GW_STRIDE, e = i - tr * GW_STRIDE;
        const int c = ax + e;
        if (e < 4 * nq && (c < 0 || c > w - 1)) {
          const int cc = c < 0 ? 0 : w - 1;
          int qsrc = (cc & ~3) - ax;
          qsrc = qsrc < 0 ? 0 : (qsrc > 4 * nq - 4 ? 4 * nq - 4 : qsrc);
          tile[tr * GW_STRIDE + e] = tile[tr * GW_STRIDE + qsrc + (cc & 3)];
        }
      }
      __syncthreads();
    }
    // 3. pixels
    int4 ycache = make_int4(-1, -1, -1, -1);
    float ey[4][4], ex[4][4];  // [lattice tap][pixel k]
    const int oy = 1 + wy0, ox = 1 + ax;
#pragma unroll
    for (int r = 0; r < RIGID_ROWS; ++r) {
      const int y = y0 + r;
      if (y >= h) break;
      // the row tables are frame-invariant: without an opaque index LICM lifts all 8 rows' taps
      // and weights out of the frame loop (64 VGPRs for the whole kernel)
      int row = wave * RIGID_ROWS + r;
      asm volatile("" : "+s"(row));
      const int4 yt4 = make_int4(s_ytap[row][0], s_ytap[row][1], s_ytap[row][2], s_ytap[row][3]);
      const float4 yc4 = make_float4(s_ycoef[row][0], s_ycoef[row][1], s_ycoef[row][2], s_ycoef[row][3]);
      if (yt4.x != ycache.x || yt4.y != ycache.y || yt4.z != ycache.z || yt4.w != ycache.w) {
        ycache = yt4;  // wave-uniform: depends on y only
        const int rows4[4] = {yt4.x, yt4.y, yt4.z, yt4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int x = xt + lane + 64 * k;
            const int xs = x < w ? x : w - 1;
            ey[i][k] = E[(int64_t)rows4[i] * w + xs];
            ex[i][k] = E[chs + (int64_t)rows4[i] * w + xs];
          }
      }
      float* orow = WRITE_FRAMES ? a.out_frames + (int64_t)f * hw + (int64_t)y * w + xt + lane : nullptr;
      if (interior) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          __builtin_amdgcn_sched_barrier(0);  // one pixel in flight (register pressure)
          float sy = dot4(yc4, ey[0][k], ey[1][k], ey[2][k], ey[3][k]);
          float sx = dot4(yc4, ex[0][k], ex[1][k], ex[2][k], ex[3][k]);
          if (!UNIT_PS) {
            sy = div_invariant(sy, a.pixel_spacing);
            sx = div_invariant(sx, a.pixel_spacing);
          }
          const float uy = grid_chain((float)y + sy, fh), ux = grid_chain((float)(xt + lane + 64 * k) + sx, fw);
          const float fy = floorf(uy), fx = floorf(ux);
          float wy[4], wx[4];
          cubic_coeffs_factored(uy - fy, wy);
          cubic_coeffs_factored(ux - fx, wx);
          const float* t0 = tile + ((int)fy - oy) * GW_STRIDE + ((int)fx - ox);
          float rowv[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float* t = t0 + i * GW_STRIDE;
            rowv[i] = gw_dot4(wx, t[0], t[1], t[2], t[3]);
          }
          const float o = gw_dot4(wy, rowv[0], rowv[1], rowv[2], rowv[3]);
          if (WRITE_FRAMES) orow[64 * k] = o;
          if (WRITE_SUM) acc[r][k] += o;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          __builtin_amdgcn_sched_barrier(0);
          const int x = xt + lane + 64 * k;
          if (x >= w) continue;
          float sy = dot4(yc4, ey[0][k], ey[1][k], ey[2][k], ey[3][k]);
          float sx = dot4(yc4, ex[0][k], ex[1][k], ex[2][k], ex[3][k]);
          if (!UNIT_PS) {
            sy = div_invariant(sy, a.pixel_spacing);
            sx = div_invariant(sx, a.pixel_spacing);
          }
          const float cy = (float)y + sy, cx = (float)x + sx;
          const bool inside = (cy >= 0.f) && (cy <= fh - 1.f) && (cx >= 0.f) && (cx <= fw - 1.f);
          const float uy = grid_chain(cy, fh), ux = grid_chain(cx, fw);
          const float fy = floorf(uy), fx = floorf(ux);
          float wy[4], wx[4];
          cubic_coeffs_factored(uy - fy, wy);
          cubic_coeffs_factored(ux - fx, wx);
          // in range by the regularity test; the clamp only keeps a garbage coordinate from
          // reading outside the LDS tile
          int ly = (int)fy - oy, lx = (int)fx - ox;
          ly = ly < 0 ? 0 : (ly > GW_ROWS - 4 ? GW_ROWS - 4 : ly);
          lx = lx < 0 ? 0 : (lx > GW_STRIDE - 4 ? GW_STRIDE - 4 : lx);
          const float* t0 = tile + ly * GW_STRIDE + lx;
          float rowv[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float* t = t0 + i * GW_STRIDE;
            rowv[i] = gw_dot4(wx, t[0], t[1], t[2], t[3]);
          }
          float o = gw_dot4(wy, rowv[0], rowv[1], rowv[2], rowv[3]);
          o = inside ? o : 0.f;
          if (WRITE_FRAMES) orow[64 * k] = o;
          if (WRITE_SUM) acc[r][k] += o;
        }
      }
    }
    __syncthreads();  // everyone is done with the tile before the next frame overwrites it
  }
  if (WRITE_SUM) {
#pragma unroll
    for (int r = 0; r < RIGID_ROWS; ++r) {
      const int y = y0 + r;
      if (y >= h) break;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = xt + lane + 64 * k;
        if (x < w) a.out_sum[(int64_t)y * w + x] = acc[r][k];  // warp_field_slow adds its tile-frames afterwards
      }
    }
  }
}

// ------------------------------------------------------------------ general warp, third version
// What the counters said about warp_field / warp_field2 (40 x 4092 x 5760, sum only, 3.0 ms): 88
// VALU instructions per pixel, almost all on the 2-cycle pipe, i.e. 1.1 ms of issue -- but a wave
// issued only every ~10 cycles (the per-pixel chain is one long dependency, 8 cycles from a result
// to its use, plus an LDS round trip per pixel) and 3 waves per SIMD were all the registers (32
// partial sums + 32 cached lattice values per lane) and the LDS (one window per workgroup) allowed;
// 37 % of the wave cycles were waits.  So: thread-level parallelism instead of registers.
//  * One workgroup of 16 waves per CU and tile; a wave owns TWO pixel rows (8 partial sums per
//    lane, ~70 VGPRs): 4 waves per SIMD.
//  * The window of frame f+1 is DMA'd into a second LDS buffer while frame f is computed (one
//    barrier per frame, no exposed DMA wait).
//  * The x-upsampled lattice rows the tile needs (E, <= 6 rows x 256 columns x 2 channels) are
//    DMA'd into LDS with the window instead of being cached in registers.
//  * Window origin, margins and the regularity verdict of every (tile, frame) come from a small
//    plan kernel, so no wave ever waits for a dependent global load inside the frame loop.
#define GW3_WAVES 16
typedef const __attribute__((address_space(3))) float* gw3_lds_cfptr;
#define GW3_RW (RIGID_WAVES * RIGID_ROWS / GW3_WAVES)  // pixel rows per wave (2)
#define GW3_EROWS 6                                     // lattice rows staged per tile
#define GW3_PLAN_MAX 128                                // frames whose plan entries are kept in LDS
#define GW3_QH 36                                       // 16-byte units (8 fp16 samples) per stage row
#define GW3_STAGE_UNITS ((((GW_ROWS * GW3_QH) + 63) / 64) * 64)

// plan[f * nt + tile] = {wy0, ax, mgy | mgx << 8 | irregular << 16, first staged lattice row R0}
__global__ __launch_bounds__(64) void warp_field_plan(FieldArgs fa, int unit_ps, int half, int4* __restrict__ plan) {
  const WarpArgs& a = fa.w;
  const int nt = a.tiles_x * a.tiles_y;
  const int tl = blockIdx.x, f = blockIdx.y;
  const int tyi = tl / a.tiles_x, txi = tl - tyi * a.tiles_x;
  const int h = a.h, w = a.w;
  const float fh = (float)h, fw = (float)w;
  const int lane = threadIdx.x;
  const int xt = txi * (RIGID_LANES * 4), yt = tyi * (RIGID_WAVES * RIGID_ROWS);
  int R0, R1, C0, C1;
  {
    int lo = 0x7fffffff, hi = -1;
    if (lane < RIGID_WAVES * RIGID_ROWS) {
      const int y = yt + lane < h ? yt + lane : h - 1;
      for (int k = 0; k < 4; ++k) {
        const int v = a.ytap[4 * y + k];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
      }
    }
    R0 = wave_min_i(lo);
    R1 = wave_max_i(hi);
    lo = 0x7fffffff;
    hi = -1;
    for (int k = 0; k < 4; ++k) {
      const int x = xt + lane + 64 * k;
      const int xs = x < w ? x : w - 1;
      for (int j = 0; j < 4; ++j) {
        const int v = fa.xtap[4 * xs + j];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
      }
    }
    C0 = wave_min_i(lo);
    C1 = wave_max_i(hi);
  }
  const int yc = (yt + 16 < h) ? yt + 16 : h - 1;
  const int xc = (xt + 128 < w) ? xt + 128 : w - 1;
  const int4 ytc = *reinterpret_cast<const int4*>(a.ytap + 4 * yc);
  const float4 ycc = *reinterpret_cast<const float4*>(a.ycoef + 4 * yc);
  const float* E = a.etab + (int64_t)f * 2 * a.GH * w;
  const int64_t chs = (int64_t)a.GH * w;
  const float* L = fa.lattice + (int64_t)f * 2 * a.GH * fa.GW;
  const int ncol = C1 - C0 + 1, nnode = (R1 - R0 + 1) * ncol;
  float lo_y = 3.0e38f, hi_y = -3.0e38f, lo_x = 3.0e38f, hi_x = -3.0e38f;
  for (int i = lane; i < nnode; i += RIGID_LANES) {
    const int R = R0 + i / ncol, Cc = C0 + i % ncol;
    const float vy = L[(int64_t)R * fa.GW + Cc], vx = L[(int64_t)(a.GH + R) * fa.GW + Cc];
    lo_y = fminf(lo_y, vy); hi_y = fmaxf(hi_y, vy);
    lo_x = fminf(lo_x, vx); hi_x = fmaxf(hi_x, vx);
  }
  const float ry = 0.5f * (wave_max_f(hi_y) - wave_min_f(lo_y)) / a.pixel_spacing;
  const float rx = 0.5f * (wave_max_f(hi_x) - wave_min_f(lo_x)) / a.pixel_spacing;
  const float ny = 3.8f * ry + 1.05f, nx = 3.8f * rx + 1.05f;
  const bool regular = (ny <= (float)GW_MG) && (nx <= (float)GW_MG) && (R1 - R0 + 1 <= GW3_EROWS);
  int4 out = make_int4(0, 0, 1 << 16, R0);
  if (regular) {
    const int mgy = (int)ceilf(ny), mgx = (int)ceilf(nx);
    const float* Ec = E + xc;
    float sy = dot4(ycc, Ec[(int64_t)ytc.x * w], Ec[(int64_t)ytc.y * w], Ec[(int64_t)ytc.z * w],
                    Ec[(int64_t)ytc.w * w]);
    float sx = dot4(ycc, Ec[chs + (int64_t)ytc.x * w], Ec[chs + (int64_t)ytc.y * w],
                    Ec[chs + (int64_t)ytc.z * w], Ec[chs + (int64_t)ytc.w * w]);
    if (!unit_ps) {
      sy = div_invariant(sy, a.pixel_spacing);
      sx = div_invariant(sx, a.pixel_spacing);
    }
    const float lim = 4.f * (fh + fw);
    const float dy = fminf(fmaxf(floorf(grid_chain((float)yc + sy, fh)) - (float)yc, -lim), lim);
    const float dx = fminf(fmaxf(floorf(grid_chain((float)xc + sx, fw)) - (float)xc, -lim), lim);
    // fp32 frames: the window starts at a 16-byte aligned column; fp16 frames: at the exact column
    // (the fp16 -> fp32 staging pass places it, warp_field3)
    const int axx = xt + (int)dx - 1 - mgx;
    out = make_int4(yt + (int)dy - 1 - mgy, half ? axx : (axx & ~3), mgy | (mgx << 8), R0);
  }
  if (lane == 0) {
    plan[(int64_t)f * nt + tl] = out;
    if (!regular) fa.flags[(int64_t)f * nt + tl] = 1;
  }
}

// RAW (N2): 1 = u8, 2 = i16 frames, staged like fp16 (16-byte units from the unit-aligned column at or left
// of the window) in the fp16 stage's space; the widening pass forms c = raw * gain - mu[f] with the gain read
// at the same (clamped) pixel, so the fp32 window holds what mc_condition_movie would have written.
// ACCUM: the sum store adds to what out_sum holds (old + tile sum, one writer per element), before the
// warp_field_slow pass adds its tile-frames: a movie warped a chunk at a time sums in launch order.
template <bool WRITE_FRAMES, bool WRITE_SUM, bool UNIT_PS, bool HALF, int RAW = 0, bool ACCUM = false>
__global__ __launch_bounds__(RIGID_LANES* GW3_WAVES, 4) void warp_field3(FieldArgs fa, const int4* __restrict__ plan) {
  static_assert(!(HALF && RAW), "fp16 or raw, not both");
  constexpr bool STAGED = HALF || RAW != 0;         // the DMA lands in a stage, a widening pass fills the window
  constexpr int SB = RAW == 1 ? 1 : 2;              // bytes per staged sample
  constexpr int UPS = 16 / SB;                      // staged samples per 16-byte unit
  const WarpArgs& a = fa.w;
  extern __shared__ __attribute__((aligned(16))) char smem_gw[];
  // fp32 frames: [window 0][window 1][E 0][E 1].  fp16 frames: [fp32 window][fp16 stage 0][fp16
  // stage 1][E 0][E 1] -- the DMA lands the raw fp16 window in a stage, one pass per frame widens it
  // into the single fp32 window (10 elements per thread; doing it per tap would be 24 instructions
  // per pixel), so the HBM side moves half the bytes and the arithmetic is unchanged.
  auto win_of = [&](int bi) { return reinterpret_cast<float4*>(smem_gw) + (STAGED ? 0 : bi) * GW_QUADS_PAD; };
  auto stage_of = [&](int bi) {
    return reinterpret_cast<float4*>(smem_gw + GW_QUADS_PAD * 16) + bi * GW3_STAGE_UNITS;
  };
  auto est_of = [&](int bi) {
    return reinterpret_cast<float*>(smem_gw + (STAGED ? GW_QUADS_PAD * 16 + 2 * GW3_STAGE_UNITS * 16
                                                    : 2 * GW_QUADS_PAD * 16)) + bi * (2 * GW3_EROWS * 256);
  };
  __shared__ int s_ytap[RIGID_WAVES * RIGID_ROWS][4];
  __shared__ float s_ycoef[RIGID_WAVES * RIGID_ROWS][4];
  const int nt = a.tiles_x * a.tiles_y;
  const int b = blockIdx.x;
  int tl = b;
  if ((nt & 7) == 0) tl = (b & 7) * (nt >> 3) + (b >> 3);
  const int tyi = tl / a.tiles_x, txi = tl - tyi * a.tiles_x;
  const int h = a.h, w = a.w;
  const float fh = (float)h, fw = (float)w;
  const int lane = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int tid = wave * RIGID_LANES + lane;
  const int xt = txi * (RIGID_LANES * 4);
  const int yt = tyi * (RIGID_WAVES * RIGID_ROWS);
  const int y0 = yt + wave * GW3_RW;
  const int64_t hw = (int64_t)h * w;
  const int64_t chs = (int64_t)a.GH * w;
  if (tid < RIGID_WAVES * RIGID_ROWS) {
    const int y = yt + tid < h ? yt + tid : h - 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s_ytap[tid][k] = a.ytap[4 * y + k];
      s_ycoef[tid][k] = a.ycoef[4 * y + k];
    }
  }
  const bool whole_tile = yt + RIGID_WAVES * RIGID_ROWS <= h && xt + RIGID_LANES * 4 <= w;
  float acc[GW3_RW][4];
#pragma unroll
  for (int r = 0; r < GW3_RW; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[r][k] = 0.f;

  // the tile's plan entries of all frames go to LDS once: a per-frame global load would put its
  // latency in front of every frame's DMA
  // (kept in LDS GW3_PLAN_MAX frames at a time: choosing between an LDS and a global load per frame
  // compiles to a flat load that waits for every outstanding DMA)
  __shared__ int4 s_plan[GW3_PLAN_MAX];
  auto stage_plan = [&](int f0) {
    for (int i = tid; f0 + i < a.nframes && i < GW3_PLAN_MAX; i += RIGID_LANES * GW3_WAVES)
      s_plan[i] = plan[(int64_t)(f0 + i) * nt + tl];
  };
  stage_plan(0);
  __syncthreads();
  auto fetch_plan = [&](int f) {
    const int4 p = s_plan[f & (GW3_PLAN_MAX - 1)];
    return make_int4(__builtin_amdgcn_readfirstlane(p.x), __builtin_amdgcn_readfirstlane(p.y),
                     __builtin_amdgcn_readfirstlane(p.z), __builtin_amdgcn_readfirstlane(p.w));
  };
  // The (window row, 16-byte unit) of each DMA unit this thread issues does not depend on the frame:
  // the divisions are done once (per frame they were 13 of the kernel's 98 VALU instructions per pixel)
  constexpr int DMA_UNITS = STAGED ? GW3_STAGE_UNITS / 64 : GW_QUADS_PAD / 64;  // wave-units of 64 lanes
  constexpr int DMA_NIT = (DMA_UNITS + GW3_WAVES - 1) / GW3_WAVES;
  constexpr int DMA_QROW = STAGED ? GW3_QH : GW_QUADS;
  int dma_tr[DMA_NIT], dma_qc[DMA_NIT];
#pragma unroll
  for (int it = 0; it < DMA_NIT; ++it) {
    const int i = wave + it * GW3_WAVES;
    const int q = i * 64 + lane;
    dma_tr[it] = i < DMA_UNITS ? q / DMA_QROW : 0x7fff;  // beyond the window: never issued
    dma_qc[it] = q - (q / DMA_QROW) * DMA_QROW;
  }
  // window + lattice rows of frame f -> LDS buffer `bi` (nothing for an irregular tile-frame)
  auto dma = [&](int f, const int4 p, int bi) {
    if (p.z >> 16) return;
    const float* fr = a.frames + (int64_t)f * hw;
    const int mgy = p.z & 255, mgx = (p.z >> 8) & 255;
    const int nrows = RIGID_WAVES * RIGID_ROWS + 3 + 2 * mgy;
    int nq = (RIGID_LANES * 4 + 6 + 2 * mgx + 3) / 4;
    nq = nq < GW_QUADS ? nq : GW_QUADS;
    if (STAGED) {  // 16-byte units of UPS samples (fp16 / i16: 8, u8: 16) from the unit-aligned column at or left of the window
      const char* frb = reinterpret_cast<const char*>(a.frames) + (int64_t)f * hw * SB;
      const int axa = p.y & ~(UPS - 1);
      const int nqh = (p.y - axa + RIGID_LANES * 4 + 3 + 2 * mgx + UPS - 1) / UPS;  // <= GW3_QH
#pragma unroll
      for (int it = 0; it < DMA_NIT; ++it) {
        if (dma_tr[it] < nrows && dma_qc[it] < nqh) {
          int r = p.x + dma_tr[it];
          r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
          int c = axa + UPS * dma_qc[it];
          c = c < 0 ? 0 : (c > w - UPS ? w - UPS : c);  // clamped units are never read (see widen)
          const unsigned off = __umul24((unsigned)r, (unsigned)w) + (unsigned)c;  // h w < 2^32 (checked by the host)
          __builtin_amdgcn_global_load_lds(frb + (size_t)off * SB, (lds_vptr)(stage_of(bi) + (wave + it * GW3_WAVES) * 64),
                                           16, 0, 0);
        }
      }
    } else {
#pragma unroll
      for (int it = 0; it < DMA_NIT; ++it) {
        if (dma_tr[it] < nrows && dma_qc[it] < nq) {
          int r = p.x + dma_tr[it];
          r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
          int c = p.y + 4 * dma_qc[it];
          c = c < 0 ? 0 : (c > w - 4 ? w - 4 : c);
          const unsigned off = __umul24((unsigned)r, (unsigned)w) + (unsigned)c;
          __builtin_amdgcn_global_load_lds(fr + off, (lds_vptr)(win_of(bi) + (wave + it * GW3_WAVES) * 64), 16, 0, 0);
        }
      }
    }
    if (wave < 2 * GW3_EROWS) {  // one 1 KiB piece per (channel, lattice row)
      const int ch = wave / GW3_EROWS, er = wave - ch * GW3_EROWS;
      int R = p.w + er;
      R = R > a.GH - 1 ? a.GH - 1 : R;
      int c = xt + 4 * lane;
      c = c > w - 4 ? w - 4 : c;  // columns beyond the image are never used
      const float* src = a.etab + (int64_t)f * 2 * chs + ch * chs + (int64_t)R * w + c;
      __builtin_amdgcn_global_load_lds(src, (lds_vptr)(est_of(bi) + (ch * GW3_EROWS + er) * 256), 16, 0, 0);
    }
  };

  // fp16: stage `bi` -> the fp32 window.  Window column j is absolute column p.y + j; border padding
  // = the clipped column, which always lies in an unclamped unit of the stage (w % 8 == 0).
  auto widen = [&](const int4 p, int bi, int f) {
    if (p.z >> 16) return;
    const int mgy = p.z & 255, mgx = (p.z >> 8) & 255;
    const int nrows = RIGID_WAVES * RIGID_ROWS + 3 + 2 * mgy;
    const int ncols = RIGID_LANES * 4 + 3 + 2 * mgx;  // <= GW_STRIDE
    const int axa = p.y & ~(UPS - 1);
    float* wn = reinterpret_cast<float*>(win_of(0));
    if constexpr (RAW != 0) {
      // raw: c = raw * gain - mu[f] (the conditioning of mc_condition_movie, in the same fp32 operations).  The
      // gain window moves with the frame's displacement, so it is read per frame, at the sample's own clamped
      // pixel; a fixed trip count keeps all of a thread's gain loads in flight together.
      constexpr int NIT = (GW_ROWS * GW_STRIDE + RIGID_LANES * GW3_WAVES - 1) / (RIGID_LANES * GW3_WAVES);
      const char* st = reinterpret_cast<const char*>(stage_of(bi));
      const float m = fa.mu[f];
      float gv[NIT], rv[NIT];
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int i = tid + it * RIGID_LANES * GW3_WAVES;
        gv[it] = 0.f;
        rv[it] = 0.f;
        if (i < nrows * ncols) {
          const int tr = i / ncols, j = i - tr * ncols;
          int xa = p.y + j;
          xa = xa < 0 ? 0 : (xa > w - 1 ? w - 1 : xa);
          int r = p.x + tr;
          r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
          gv[it] = fa.gain[__umul24((unsigned)r, (unsigned)w) + (unsigned)xa];
          const char* sp = st + tr * (16 * GW3_QH) + (xa - axa) * SB;
          rv[it] = RAW == 1 ? (float)*reinterpret_cast<const unsigned char*>(sp) : (float)*reinterpret_cast<const short*>(sp);
        }
      }
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int i = tid + it * RIGID_LANES * GW3_WAVES;
        if (i < nrows * ncols) {
          const int tr = i / ncols, j = i - tr * ncols;
          wn[tr * GW_STRIDE + j] = rv[it] * gv[it] - m;
        }
      }
    } else {
      const _Float16* st = reinterpret_cast<const _Float16*>(stage_of(bi));
      for (int i = tid; i < nrows * ncols; i += RIGID_LANES * GW3_WAVES) {
        const int tr = i / ncols, j = i - tr * ncols;
        int xa = p.y + j;
        xa = xa < 0 ? 0 : (xa > w - 1 ? w - 1 : xa);
        wn[tr * GW_STRIDE + j] = (float)st[tr * (8 * GW3_QH) + (xa - axa)];
      }
    }
  };

  int4 pc = fetch_plan(0);
  dma(0, pc, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (STAGED) {
    widen(pc, 0, 0);
    __syncthreads();
  }
  for (int f = 0; f < a.nframes; ++f) {
    const int bi = f & 1;
    int4 pn = pc;
    if (f + 1 < a.nframes) {
      if (((f + 1) & (GW3_PLAN_MAX - 1)) == 0) {  // next block of plan entries (every thread already holds pc)
        __syncthreads();
        stage_plan(f + 1);
        __syncthreads();
      }
      pn = fetch_plan(f + 1);
      dma(f + 1, pn, bi ^ 1);  // lands under this frame's arithmetic
    }
    if (!(pc.z >> 16)) {
      const int wy0 = pc.x, ax = pc.y, mgy = pc.z & 255, mgx = (pc.z >> 8) & 255, R0 = pc.w;
      const int nrows = RIGID_WAVES * RIGID_ROWS + 3 + 2 * mgy;
      int nq = (RIGID_LANES * 4 + 6 + 2 * mgx + 3) / 4;
      nq = nq < GW_QUADS ? nq : GW_QUADS;
      float* const tile = reinterpret_cast<float*>(win_of(bi));
      const float* const es = est_of(bi);
      if (!STAGED && (ax < 0 || ax + 4 * nq > w)) {  // border padding: clipped columns (edge tiles only)
        for (int i = tid; i < nrows * GW_STRIDE; i += RIGID_LANES * GW3_WAVES) {
          const int tr = i / GW_STRIDE, e = i - tr * GW_STRIDE;
          const int c = ax + e;
          if (e < 4 * nq && (c < 0 || c > w - 1)) {
            const int cc = c < 0 ? 0 : w - 1;
            int qsrc = (cc & ~3) - ax;
            qsrc = qsrc < 0 ? 0 : (qsrc > 4 * nq - 4 ? 4 * nq - 4 : qsrc);
            tile[tr * GW_STRIDE + e] = tile[tr * GW_STRIDE + qsrc + (cc & 3)];
          }
        }
        __syncthreads();
      }
      const bool interior_rt = whole_tile && wy0 >= 0 && wy0 + nrows <= h && ax >= 0 &&
                               ax + (STAGED ? RIGID_LANES * 4 + 3 + 2 * mgx : 4 * nq) <= w;
      const int oy = 1 + wy0, ox = 1 + ax;
      const unsigned tap_base = (unsigned)(uintptr_t)(lds_vptr)tile - 4u * (unsigned)(oy * GW_STRIDE + ox);
      // The tile-frame's two bodies are separate instantiations: the interior one (no zero-outside
      // test, no column predicate) is straight-line code for all of a wave's pixels, so the LDS reads
      // of one pixel are scheduled under the arithmetic of another instead of every pixel ending in an
      // exec-mask branch.
      auto pixels = [&](auto interior_tag) {
        constexpr bool interior = decltype(interior_tag)::value;
      // What the counters say (profiles/r03_warp_field3_pmc.txt, 40 x 4092 x 5760 sum only): 87 VALU
      // instructions per pixel at ~4.4 cycles each with 4 waves per SIMD, LDS address pipe 52 % busy.
      // Measured alternatives, same results, none faster: 2 or 4 pixels of a lane in flight together
      // (GW3_ILP), the wave's two rows statement by statement, the y/x sides of the chain or row pairs
      // of the taps on 2-float vectors (a v_pk_*_f32 instruction costs 1.35-1.6 x a scalar one here,
      // scripts/ubench/pk_rate.hip, and the pairs have to be built with moves: 3.24 ms against 2.98).
      // Removing 11 % of the instructions (frame-invariant DMA indices, v_fract / v_cvt_flr, one tap
      // address) bought 4 % of the time.
      if constexpr (interior) {
        // Interior tile-frames (all but the frame's rim): GW3_ILP pixels of a lane side by side -- their
        // chains (shift, coordinate, weights, address) are independent, so a dependent instruction of one
        // issues behind an instruction of the other -- then all their taps in one batch of LDS reads.
        // Coordinates are positive here: v_fract_f32 IS u - floor(u) (exact either way) and
        // v_cvt_flr_i32_f32 is the floor as an integer; the tap address is one 24-bit multiply-add and one
        // shift-add from a per-frame base that holds the window origin; the 16 taps are single reads with
        // 16-bit immediate offsets from that ONE address (paired into ds_read2_b32, whose 8-bit offsets do
        // not reach the next window row, they cost 6 address adds per pixel).
#pragma unroll
        for (int r = 0; r < GW3_RW; ++r) {
          const int y = y0 + r;
          const int row = wave * GW3_RW + r;
          const float4 yc4 = make_float4(s_ycoef[row][0], s_ycoef[row][1], s_ycoef[row][2], s_ycoef[row][3]);
          const float* e0 = es + (s_ytap[row][0] - R0) * 256 + lane;
          const float* e1 = es + (s_ytap[row][1] - R0) * 256 + lane;
          const float* e2 = es + (s_ytap[row][2] - R0) * 256 + lane;
          const float* e3 = es + (s_ytap[row][3] - R0) * 256 + lane;
          float* orow = WRITE_FRAMES ? a.out_frames + (int64_t)f * hw + (int64_t)y * w + xt + lane : nullptr;
#pragma unroll
          for (int k0 = 0; k0 < 4; k0 += GW3_ILP) {
            float wy[GW3_ILP][4], wx[GW3_ILP][4], tp[GW3_ILP][16];
            gw3_lds_cfptr t0[GW3_ILP];
#pragma unroll
            for (int q = 0; q < GW3_ILP; ++q) {
              const int k = k0 + q;
              float sy = dot4(yc4, e0[64 * k], e1[64 * k], e2[64 * k], e3[64 * k]);
              float sx = dot4(yc4, e0[64 * k + GW3_EROWS * 256], e1[64 * k + GW3_EROWS * 256],
                              e2[64 * k + GW3_EROWS * 256], e3[64 * k + GW3_EROWS * 256]);
              if (!UNIT_PS) {
                sy = div_invariant(sy, a.pixel_spacing);
                sx = div_invariant(sx, a.pixel_spacing);
              }
              const float uy = grid_chain((float)y + sy, fh), ux = grid_chain((float)(xt + lane + 64 * k) + sx, fw);
              cubic_coeffs_factored(__builtin_amdgcn_fractf(uy), wy[q]);
              cubic_coeffs_factored(__builtin_amdgcn_fractf(ux), wx[q]);
              int iy, ix;
              asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(iy) : "v"(uy));
              asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ix) : "v"(ux));
              t0[q] = (gw3_lds_cfptr)(uintptr_t)(__umul24((unsigned)iy, 4u * GW_STRIDE) + tap_base + ((unsigned)ix << 2));
            }
#define GW3_RD(i, j) "ds_read_b32 %" #i ", %16 offset:%c" #j "\n"
#pragma unroll
            for (int q = 0; q < GW3_ILP; ++q)
              asm volatile(GW3_RD(0, 17) GW3_RD(1, 18) GW3_RD(2, 19) GW3_RD(3, 20) GW3_RD(4, 21) GW3_RD(5, 22) GW3_RD(6, 23)
                           GW3_RD(7, 24) GW3_RD(8, 25) GW3_RD(9, 26) GW3_RD(10, 27) GW3_RD(11, 28) GW3_RD(12, 29)
                           GW3_RD(13, 30) GW3_RD(14, 31) GW3_RD(15, 32)
                           : "=&v"(tp[q][0]), "=&v"(tp[q][1]), "=&v"(tp[q][2]), "=&v"(tp[q][3]), "=&v"(tp[q][4]),
                             "=&v"(tp[q][5]), "=&v"(tp[q][6]), "=&v"(tp[q][7]), "=&v"(tp[q][8]), "=&v"(tp[q][9]),
                             "=&v"(tp[q][10]), "=&v"(tp[q][11]), "=&v"(tp[q][12]), "=&v"(tp[q][13]), "=&v"(tp[q][14]),
                             "=&v"(tp[q][15])
                           : "v"(t0[q]), "n"(0), "n"(4), "n"(8), "n"(12), "n"(4 * GW_STRIDE), "n"(4 * GW_STRIDE + 4),
                             "n"(4 * GW_STRIDE + 8), "n"(4 * GW_STRIDE + 12), "n"(8 * GW_STRIDE), "n"(8 * GW_STRIDE + 4),
                             "n"(8 * GW_STRIDE + 8), "n"(8 * GW_STRIDE + 12), "n"(12 * GW_STRIDE), "n"(12 * GW_STRIDE + 4),
                             "n"(12 * GW_STRIDE + 8), "n"(12 * GW_STRIDE + 12)
                           : "memory");
#undef GW3_RD
            // one wait for the batch; the operand lists tie every tap to it
#pragma unroll
            for (int q = 0; q < GW3_ILP; ++q)
              asm volatile("s_waitcnt lgkmcnt(0)"
                           : "+v"(tp[q][0]), "+v"(tp[q][1]), "+v"(tp[q][2]), "+v"(tp[q][3]), "+v"(tp[q][4]), "+v"(tp[q][5]),
                             "+v"(tp[q][6]), "+v"(tp[q][7]), "+v"(tp[q][8]), "+v"(tp[q][9]), "+v"(tp[q][10]),
                             "+v"(tp[q][11]), "+v"(tp[q][12]), "+v"(tp[q][13]), "+v"(tp[q][14]), "+v"(tp[q][15])
                           :: "memory");
#pragma unroll
            for (int q = 0; q < GW3_ILP; ++q) {
              float rowv[4];
#pragma unroll
              for (int i = 0; i < 4; ++i)
                rowv[i] = gw_dot4(wx[q], tp[q][4 * i], tp[q][4 * i + 1], tp[q][4 * i + 2], tp[q][4 * i + 3]);
              const float o = gw_dot4(wy[q], rowv[0], rowv[1], rowv[2], rowv[3]);
              if (WRITE_FRAMES) orow[64 * (k0 + q)] = o;
              if (WRITE_SUM) acc[r][k0 + q] += o;
            }
          }
        }
      } else
#pragma unroll
      for (int r = 0; r < GW3_RW; ++r) {
        const int y = y0 + r;
        if (!interior && y >= h) break;
        const int row = wave * GW3_RW + r;
        const float4 yc4 = make_float4(s_ycoef[row][0], s_ycoef[row][1], s_ycoef[row][2], s_ycoef[row][3]);
        const float* e0 = es + (s_ytap[row][0] - R0) * 256 + lane;
        const float* e1 = es + (s_ytap[row][1] - R0) * 256 + lane;
        const float* e2 = es + (s_ytap[row][2] - R0) * 256 + lane;
        const float* e3 = es + (s_ytap[row][3] - R0) * 256 + lane;
        float* orow = WRITE_FRAMES ? a.out_frames + (int64_t)f * hw + (int64_t)y * w + xt + lane : nullptr;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int x = xt + lane + 64 * k;
          if (!interior && x >= w) continue;
          float sy = dot4(yc4, e0[64 * k], e1[64 * k], e2[64 * k], e3[64 * k]);
          float sx = dot4(yc4, e0[64 * k + GW3_EROWS * 256], e1[64 * k + GW3_EROWS * 256],
                          e2[64 * k + GW3_EROWS * 256], e3[64 * k + GW3_EROWS * 256]);
          if (!UNIT_PS) {
            sy = div_invariant(sy, a.pixel_spacing);
            sx = div_invariant(sx, a.pixel_spacing);
          }
          const float cy = (float)y + sy, cx = (float)x + sx;
          const float uy = grid_chain(cy, fh), ux = grid_chain(cx, fw);
          float wy[4], wx[4];
          float rowv[4];
          const float fy = floorf(uy), fx = floorf(ux);
          cubic_coeffs_factored(uy - fy, wy);
          cubic_coeffs_factored(ux - fx, wx);
          int ly = (int)fy - oy, lx = (int)fx - ox;
          const bool inside = (cy >= 0.f) && (cy <= fh - 1.f) && (cx >= 0.f) && (cx <= fw - 1.f);
          // in range by the regularity test; the clamp only keeps a garbage coordinate from
          // reading outside the LDS tile
          ly = ly < 0 ? 0 : (ly > GW_ROWS - 4 ? GW_ROWS - 4 : ly);
          lx = lx < 0 ? 0 : (lx > GW_STRIDE - 4 ? GW_STRIDE - 4 : lx);
          const float* t0 = tile + ly * GW_STRIDE + lx;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float* t = t0 + i * GW_STRIDE;
            rowv[i] = gw_dot4(wx, t[0], t[1], t[2], t[3]);
          }
          float o = gw_dot4(wy, rowv[0], rowv[1], rowv[2], rowv[3]);
          o = inside ? o : 0.f;
          if (WRITE_FRAMES) orow[64 * k] = o;
          if (WRITE_SUM) acc[r][k] += o;
        }
      }
      };
      if (interior_rt) pixels(std::true_type{});
      else pixels(std::false_type{});
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // DMA of f+1 (and this frame's stores)
    __syncthreads();  // buffer bi is free again, buffer bi^1 is complete
    if (STAGED && f + 1 < a.nframes) {
      widen(pn, bi ^ 1, f + 1);
      __syncthreads();
    }
    pc = pn;
  }
  if (WRITE_SUM) {
#pragma unroll
    for (int r = 0; r < GW3_RW; ++r) {
      const int y = y0 + r;
      if (y >= h) break;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = xt + lane + 64 * k;
        if (x < w) {  // warp_field_slow adds its tile-frames afterwards
          float* dst = a.out_sum + (int64_t)y * w + x;
          *dst = ACCUM ? *dst + acc[r][k] : acc[r][k];
        }
      }
    }
  }
}

// Tile-frames warp_field2 / warp_field3 flagged as irregular: generic per-pixel gathers from global
// memory (border padding by clipping every tap coordinate).  One workgroup per tile, so
// the += on out_sum cannot race.
// RAW (N2): u8 / i16 frames, every tap conditioned as raw * gain - mu[f] at its clamped pixel (the zero
// outside the frame stays the conditioned domain's zero).
template <bool UNIT_PS, bool HALF = false, int RAW = 0>
__global__ __launch_bounds__(RIGID_LANES* RIGID_WAVES) void warp_field_slow(FieldArgs fa, int write_frames,
                                                                           int write_sum) {
  const WarpArgs& a = fa.w;
  const int nt = a.tiles_x * a.tiles_y;
  const int tl = blockIdx.x;
  bool any = false;
  for (int f = 0; f < a.nframes; ++f) any = any || fa.flags[(int64_t)f * nt + tl];
  if (!any) return;
  const int tyi = tl / a.tiles_x, txi = tl - tyi * a.tiles_x;
  const int h = a.h, w = a.w;
  const float fh = (float)h, fw = (float)w;
  const int64_t hw = (int64_t)h * w;
  const int64_t chs = (int64_t)a.GH * w;
  const int xt = txi * (RIGID_LANES * 4), yt = tyi * (RIGID_WAVES * RIGID_ROWS);
  for (int i = threadIdx.y * RIGID_LANES + threadIdx.x; i < RIGID_LANES * 4 * RIGID_WAVES * RIGID_ROWS;
       i += RIGID_LANES * RIGID_WAVES) {
    const int y = yt + i / (RIGID_LANES * 4), x = xt + i % (RIGID_LANES * 4);
    if (y >= h || x >= w) continue;
    const int4 yt4 = *reinterpret_cast<const int4*>(a.ytap + 4 * y);
    const float4 yc4 = *reinterpret_cast<const float4*>(a.ycoef + 4 * y);
    float accp = 0.f;
    for (int f = 0; f < a.nframes; ++f) {
      if (!fa.flags[(int64_t)f * nt + tl]) continue;
      const float* fr = a.frames + (int64_t)f * hw;
      const _Float16* frh = reinterpret_cast<const _Float16*>(a.frames) + (int64_t)f * hw;
      const float* E = a.etab + (int64_t)f * 2 * a.GH * w + x;
      float sy = dot4(yc4, E[(int64_t)yt4.x * w], E[(int64_t)yt4.y * w], E[(int64_t)yt4.z * w],
                      E[(int64_t)yt4.w * w]);
      float sx = dot4(yc4, E[chs + (int64_t)yt4.x * w], E[chs + (int64_t)yt4.y * w],
                      E[chs + (int64_t)yt4.z * w], E[chs + (int64_t)yt4.w * w]);
      if (!UNIT_PS) {
        sy = div_invariant(sy, a.pixel_spacing);
        sx = div_invariant(sx, a.pixel_spacing);
      }
      const float cy = (float)y + sy, cx = (float)x + sx;
      const bool inside = (cy >= 0.f) && (cy <= fh - 1.f) && (cx >= 0.f) && (cx <= fw - 1.f);
      const float uy = grid_chain(cy, fh), ux = grid_chain(cx, fw);
      const float fy = floorf(uy), fx = floorf(ux);
      float wy[4], wx[4];
      cubic_coeffs_fast(uy - fy, wy);
      cubic_coeffs_fast(ux - fx, wx);
      float rowv[4];
      for (int ii = 0; ii < 4; ++ii) {
        const float ty = fminf(fmaxf(fy + (float)(ii - 1), 0.f), fh - 1.f);
        const int64_t ro = (int64_t)(int)ty * w;
        float t4[4];
        for (int j = 0; j < 4; ++j) {
          const int64_t o = ro + (int)fminf(fmaxf(fx + (float)(j - 1), 0.f), fw - 1.f);
          if constexpr (RAW == 1) t4[j] = (float)reinterpret_cast<const unsigned char*>(a.frames)[f * hw + o] * fa.gain[o] - fa.mu[f];
          else if constexpr (RAW == 2) t4[j] = (float)reinterpret_cast<const short*>(a.frames)[f * hw + o] * fa.gain[o] - fa.mu[f];
          else t4[j] = HALF ? (float)frh[o] : fr[o];
        }
        rowv[ii] = gw_dot4(wx, t4[0], t4[1], t4[2], t4[3]);
      }
      float o = gw_dot4(wy, rowv[0], rowv[1], rowv[2], rowv[3]);
      o = inside ? o : 0.f;
      if (write_frames) a.out_frames[(int64_t)f * hw + (int64_t)y * w + x] = o;
      accp += o;
    }
    if (write_sum) a.out_sum[(int64_t)y * w + x] += accp;
  }
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
// The field warp's scratch: etab | ytap | ycoef | xtap | xcoef | flags | plan, carved from `scratch`
// (16-byte aligned): one flag byte and one 16-byte plan entry per (frame, 256 x 32 tile).
struct FieldScratch {
  float* etab;   // [f][2][GH][w]
  int* ytap;     // [h][4]
  float* ycoef;  // [h][4]
  int* xtap;     // [w][4]
  float* xcoef;  // [w][4]
  unsigned char* flags;
  int4* plan;
  int64_t flag_bytes;
  int64_t bytes;  // what mc_warp_scratch_bytes reports
};
static FieldScratch field_scratch(float* scratch, int nframes, int h, int w, int GH) {
  const int64_t tx = (w + RIGID_LANES * 4 - 1) / (RIGID_LANES * 4);
  const int64_t ty = (h + RIGID_WAVES * RIGID_ROWS - 1) / (RIGID_WAVES * RIGID_ROWS);
  const int64_t etab_floats = (((int64_t)nframes * 2 * GH * w) + 3) & ~(int64_t)3;  // keep the int4 tables aligned
  FieldScratch t;
  t.flag_bytes = ((int64_t)nframes * tx * ty + 15) & ~(int64_t)15;
  uintptr_t p = reinterpret_cast<uintptr_t>(scratch);
  auto take = [&p](int64_t nbytes) {
    void* q = reinterpret_cast<void*>(p);
    p += (uintptr_t)nbytes;
    return q;
  };
  t.etab = static_cast<float*>(take(etab_floats * 4));
  t.ytap = static_cast<int*>(take(16 * (int64_t)h));
  t.ycoef = static_cast<float*>(take(16 * (int64_t)h));
  t.xtap = static_cast<int*>(take(16 * (int64_t)w));
  t.xcoef = static_cast<float*>(take(16 * (int64_t)w));
  t.flags = static_cast<unsigned char*>(take(t.flag_bytes));
  t.plan = static_cast<int4*>(take(16 * t.flag_bytes));
  t.bytes = (int64_t)(p - reinterpret_cast<uintptr_t>(scratch));
  return t;
}

// the per-axis tap tables and the x-upsampled lattice E of `nframes` lattices
static void field_tables_launch(const float* lattice, int nframes, int h, int w, int GH, int GW, const FieldScratch& t,
                                hipStream_t s) {
  hipLaunchKernelGGL(warp_axis_tables, dim3((h + 255) / 256), dim3(256), 0, s, h, GH, t.ytap, t.ycoef);
  hipLaunchKernelGGL(warp_axis_tables, dim3((w + 255) / 256), dim3(256), 0, s, w, GW, t.xtap, t.xcoef);
  hipLaunchKernelGGL(warp_etab, dim3((w + 255) / 256, nframes * 2 * GH), dim3(256), 0, s, lattice, GH, GW, w,
                     (const int*)t.xtap, (const float*)t.xcoef, t.etab);
}

// Route rules.  warp_field3 stages <= GW3_EROWS lattice rows per tile: 32 pixel rows must span <= 1.5
// lattice cells (always for the reference's 10 nodes per patch; not for a per-pixel lattice) ...
static bool field3_lattice_ok(int h, int GH) { return (int64_t)32 * (GH - 1) * 2 <= (int64_t)3 * (h - 1); }
// ... and it addresses a frame with 32-bit element offsets built by 24-bit multiplies
static bool field3_small32(int h, int w) { return h < (1 << 24) && w < (1 << 24) && (int64_t)h * w < ((int64_t)1 << 31); }

// arguments of the tiled kernels (256 x 32 tiles); gain / mu for raw frames only
static FieldArgs field_args(const void* frames, int nframes, int h, int w, const float* lattice, int GH, int GW,
                            float pixel_spacing, const FieldScratch& t, float* out_frames, float* out_sum,
                            const float* gain, const float* mu) {
  FieldArgs fa;
  WarpArgs& a = fa.w;
  a.frames = static_cast<const float*>(frames); a.nframes = nframes; a.h = h; a.w = w; a.GH = GH; a.etab = t.etab;
  a.ytap = t.ytap; a.ycoef = t.ycoef; a.pixel_spacing = pixel_spacing;
  a.out_frames = out_frames; a.out_sum = out_sum;
  a.tiles_x = (w + RIGID_LANES * 4 - 1) / (RIGID_LANES * 4);
  a.tiles_y = (h + RIGID_WAVES * RIGID_ROWS - 1) / (RIGID_WAVES * RIGID_ROWS);
  fa.lattice = lattice; fa.xtap = t.xtap; fa.GW = GW; fa.flags = t.flags; fa.gain = gain; fa.mu = mu;
  return fa;
}

// warp_field_slow over the tile-frames the tiled kernel flagged
template <bool UNIT_PS, bool HALF, int RAW>
static void field_slow_launch(const FieldArgs& fa, hipStream_t s) {
  hipLaunchKernelGGL((warp_field_slow<UNIT_PS, HALF, RAW>), dim3(fa.w.tiles_x * fa.w.tiles_y), dim3(RIGID_LANES, RIGID_WAVES),
                     0, s, fa, fa.w.out_frames ? 1 : 0, fa.w.out_sum ? 1 : 0);
}

// plan, warp_field3, warp_field_slow.  RAW 0: fp32 or (half) fp16 frames; 1 / 2: u8 / i16 frames, which alone
// may accumulate.  fp16 and raw windows start at the exact column (the widening pass places them).
template <int RAW>
static void field3_launch(const FieldArgs& fa, const FieldScratch& t, bool half, bool accumulate, hipStream_t s) {
  const WarpArgs& a = fa.w;
  const bool staged = half || RAW != 0;
  const int4* plan = t.plan;
  const dim3 grid(a.tiles_x * a.tiles_y), block3(RIGID_LANES, GW3_WAVES);
  const size_t lds3 = (staged ? (size_t)GW_QUADS_PAD * 16 + (size_t)2 * GW3_STAGE_UNITS * 16 : (size_t)2 * GW_QUADS_PAD * 16) +
                      (size_t)2 * 2 * GW3_EROWS * 256 * 4;
  mc_pick(a.pixel_spacing == 1.0f, [&](auto U) {
    hipLaunchKernelGGL(warp_field_plan, dim3(a.tiles_x * a.tiles_y, a.nframes), dim3(64), 0, s, fa, U.value ? 1 : 0,
                       staged ? 1 : 0, t.plan);
    auto go = [&](auto F, auto S, auto H, auto A) {
      auto k = warp_field3<F.value, S.value, U.value, H.value, RAW, A.value>;
      (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3);
      hipLaunchKernelGGL(k, grid, block3, lds3, s, fa, plan);
    };
    if constexpr (RAW != 0) {
      mc_pick_outputs_accum(a.out_frames != nullptr, a.out_sum != nullptr, accumulate,
                            [&](auto F, auto S, auto A) { go(F, S, std::false_type{}, A); });
      field_slow_launch<U.value, false, RAW>(fa, s);
    } else {
      mc_pick(half, [&](auto H) {
        mc_pick_outputs(a.out_frames != nullptr, a.out_sum != nullptr, [&](auto F, auto S) { go(F, S, H, std::false_type{}); });
        field_slow_launch<U.value, H.value, 0>(fa, s);
      });
    }
  });
}

// N2: the deformation-field warp fed from the RAW movie (warp_field3 / warp_field_slow with RAW = 1 / 2): the same
// tables, plan and tiles as mc_warp_frames_t for fp16 frames, the raw window conditioned in the widening pass.
static int warp_frames_raw_impl(const void* raw, int storage, const float* gain, const float* mu, int nframes, int h,
                                int w, const float* lattice, int GH, int GW, float pixel_spacing, float* scratch,
                                float* out_frames, float* out_sum, bool accumulate, void* stream) {
  if (storage != MC_STORE_U8 && storage != MC_STORE_I16) return MC_ERR_UNSUPPORTED;
  if (!raw || !gain || !mu || !lattice || !scratch || (!out_frames && !out_sum)) return MC_ERR_ARG;
  if (nframes < 1 || h < 2 || w < 2 || GH < 1 || GW < 1 || !(pixel_spacing > 0.f)) return MC_ERR_ARG;
  if (((uintptr_t)scratch) & 15) return MC_ERR_ARG;
  const int ups = storage == MC_STORE_U8 ? 16 : 8;  // samples per 16-byte DMA unit: rows of whole units
  if ((w % ups) || (((uintptr_t)raw) & 15) || (((uintptr_t)gain) & 3) || !field3_small32(h, w) || !field3_lattice_ok(h, GH))
    return MC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const FieldScratch t = field_scratch(scratch, nframes, h, w, GH);
  field_tables_launch(lattice, nframes, h, w, GH, GW, t, s);
  const FieldArgs fa = field_args(raw, nframes, h, w, lattice, GH, GW, pixel_spacing, t, out_frames, out_sum, gain, mu);
  hipError_t e = hipMemsetAsync(t.flags, 0, (size_t)t.flag_bytes, s);
  if (e != hipSuccess) return (int)e;
  if (storage == MC_STORE_U8) field3_launch<1>(fa, t, false, accumulate, s);
  else field3_launch<2>(fa, t, false, accumulate, s);
  return mc_check_launch();
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

int mc_warp_frames_t(const void* frames, int storage, int nframes, int h, int w, const float* lattice,
                     int GH, int GW, float pixel_spacing, float* scratch, float* out_frames, float* out_sum,
                     void* stream) {
  if (storage != MC_STORE_F32 && storage != MC_STORE_F16) return MC_ERR_UNSUPPORTED;
  const bool half = storage == MC_STORE_F16;
  // fp16 frames take the LDS-staged kernel only: 16-byte rows of 8 samples and the reference's sparse
  // lattice (10 nodes per patch); anything else is MC_ERR_UNSUPPORTED and the caller widens the stack
  if (half && ((w % 8) || (((uintptr_t)frames) & 15) || !field3_lattice_ok(h, GH))) return MC_ERR_UNSUPPORTED;
  if (!frames || !lattice || !scratch || (!out_frames && !out_sum)) return MC_ERR_ARG;
  if (nframes < 1 || h < 2 || w < 2 || GH < 1 || GW < 1 || !(pixel_spacing > 0.f)) return MC_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (((uintptr_t)scratch) & 15) return MC_ERR_ARG;
  const FieldScratch t = field_scratch(scratch, nframes, h, w, GH);
  field_tables_launch(lattice, nframes, h, w, GH, GW, t, s);
  FieldArgs fa = field_args(frames, nframes, h, w, lattice, GH, GW, pixel_spacing, t, out_frames, out_sum, nullptr, nullptr);
  if ((w % 4 == 0) && ((((uintptr_t)frames) & 15) == 0)) {
    hipError_t e = hipMemsetAsync(t.flags, 0, (size_t)t.flag_bytes, s);
    if (e != hipSuccess) return (int)e;
    if (field3_small32(h, w) && field3_lattice_ok(h, GH)) {
      field3_launch<0>(fa, t, half, false, s);
      return mc_check_launch();
    }
    // dense lattices (and frames beyond 32-bit offsets) fall back to warp_field2, which reads fp32 only
    if (half) return MC_ERR_UNSUPPORTED;
    const dim3 grid(fa.w.tiles_x * fa.w.tiles_y), block(RIGID_LANES, RIGID_WAVES);
    mc_pick(pixel_spacing == 1.0f, [&](auto U) {
      mc_pick_outputs(out_frames != nullptr, out_sum != nullptr, [&](auto F, auto S) {
        hipLaunchKernelGGL((warp_field2<F.value, S.value, U.value>), grid, block, (size_t)GW_QUADS_PAD * 16, s, fa);
      });
      field_slow_launch<U.value, false, 0>(fa, s);
    });
    return mc_check_launch();
  }
  // rows that are not whole float4 quads (or an unaligned stack): the first, untiled kernel.  It reads
  // fp32 only -- an fp16 stack never gets here (its rows are whole 8-sample units, checked above), and
  // must not: the kernel would read twice the buffer's bytes
  if (half) return MC_ERR_UNSUPPORTED;
  WarpArgs& a = fa.w;
  a.tiles_x = (w + WARP_TX * WARP_PX - 1) / (WARP_TX * WARP_PX);
  a.tiles_y = (h + WARP_TY * WARP_ROWS - 1) / (WARP_TY * WARP_ROWS);
  const dim3 grid(a.tiles_x * a.tiles_y), block(WARP_TX, WARP_TY);
  mc_pick(pixel_spacing == 1.0f, [&](auto U) {
    mc_pick_outputs(out_frames != nullptr, out_sum != nullptr, [&](auto F, auto S) {
      hipLaunchKernelGGL((warp_main<F.value, S.value, U.value>), grid, block, 0, s, a);
    });
  });
  return mc_check_launch();
}

int mc_warp_frames(const float* frames, int nframes, int h, int w, const float* lattice, int GH,
                   int GW, float pixel_spacing, float* scratch, float* out_frames, float* out_sum,
                   void* stream) {
  return mc_warp_frames_t(frames, MC_STORE_F32, nframes, h, w, lattice, GH, GW, pixel_spacing, scratch,
                          out_frames, out_sum, stream);
}

int mc_warp_frames_raw(const void* raw, int storage, const float* gain, const float* mu, int nframes, int h, int w,
                       const float* lattice, int GH, int GW, float pixel_spacing, float* scratch, float* out_frames,
                       float* out_sum, void* stream) {
  return warp_frames_raw_impl(raw, storage, gain, mu, nframes, h, w, lattice, GH, GW, pixel_spacing, scratch, out_frames,
                              out_sum, false, stream);
}

int mc_warp_frames_raw_accumulate(const void* raw, int storage, const float* gain, const float* mu, int nframes, int h,
                                  int w, const float* lattice, int GH, int GW, float pixel_spacing, float* scratch,
                                  float* out_frames, float* out_sum, void* stream) {
  if (!raw || !gain || !mu || !lattice || !scratch || !out_sum) return MC_ERR_ARG;
  return warp_frames_raw_impl(raw, storage, gain, mu, nframes, h, w, lattice, GH, GW, pixel_spacing, scratch, out_frames,
                              out_sum, true, stream);
}

int mc_pixel_shifts(const float* lattice, int GH, int GW, int h, int w, float pixel_spacing,
                    float* scratch, float* out, void* stream) {
  if (!lattice || !scratch || !out || h < 2 || w < 2 || GH < 1 || GW < 1 || !(pixel_spacing > 0.f))
    return MC_ERR_ARG;
  if (((uintptr_t)scratch) & 15) return MC_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const FieldScratch t = field_scratch(scratch, 1, h, w, GH);
  field_tables_launch(lattice, 1, h, w, GH, GW, t, s);
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
