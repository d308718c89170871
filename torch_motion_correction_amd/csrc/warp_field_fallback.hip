// The two fallback kernels of the deformation-field warp, each reached through one narrow route of
// mc_warp_frames_t (warp_field.hip has the rule), fp32 frames only:
//   warp_main    rows that are not whole float4 quads, or a stack off a 16-byte boundary: untiled, every
//                thread gathers its taps from global memory through a register window;
//   warp_field2  lattices too dense for warp_field3's staged lattice rows (or frames beyond 32-bit
//                offsets): the LDS-window kernel with the plan worked out inside its own frame loop.
//
// No FMA contraction in this object: warp_field_common.h says why.
#include "warp_field_common.h"
#pragma clang fp contract(off)

// Measured setting (DESIGN.md section 4 has the alternatives)
#define GW2_MINW 3  // warp_field2: workgroups per CU the register budget is held to

// ------------------------------------------------------------------ warp_main: register window, global gathers
#define WARP_TX 32   // threads across, 4 px each -> 128 px
#define WARP_TY 8    // thread rows, 2 adjacent pixel rows each -> 16 rows
#define WARP_PX 4
#define WARP_ROWS 2

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));  // dword-aligned 16-B load

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

// ------------------------------------------------------------------ warp_field2: LDS window, plan in the frame loop
// The tiling, window and per-pixel chain that warp_field_common.h describes, one window per workgroup:
//  * the window margin follows the field: mg = ceil(3.8 rho + 1.05) per axis and tile-frame (2 for
//    the smooth fields of real movies) instead of the full GW_MG, lanes outside the needed window
//    issue no DMA (window bytes 1.6x -> 1.3x of the tile);
//  * 3 workgroups per CU (one 52 KB window each), so a workgroup's DMA wait hides under two others;
//  * tile-frames whose window lies inside the image (all but the frame's rim) take a body without
//    the zero-outside test and without index clamps;
//  * a thread caches its 4 px x 4 lattice rows x 2 channels of E in registers while consecutive pixel
//    rows use the same lattice rows (they almost always do).
// Unlike warp_field3 it takes any lattice density and 64-bit frame offsets.
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

// ------------------------------------------------------------------ host side
void mc_warp_main_launch(WarpArgs a, hipStream_t s) {
  a.tiles_x = (a.w + WARP_TX * WARP_PX - 1) / (WARP_TX * WARP_PX);
  a.tiles_y = (a.h + WARP_TY * WARP_ROWS - 1) / (WARP_TY * WARP_ROWS);
  const dim3 grid(a.tiles_x * a.tiles_y), block(WARP_TX, WARP_TY);
  mc_pick(a.pixel_spacing == 1.0f, [&](auto U) {
    mc_pick_outputs(a.out_frames != nullptr, a.out_sum != nullptr, [&](auto F, auto S) {
      hipLaunchKernelGGL((warp_main<F.value, S.value, U.value>), grid, block, 0, s, a);
    });
  });
}

void mc_warp_field2_launch(const FieldArgs& fa, hipStream_t s) {
  const dim3 grid(fa.w.tiles_x * fa.w.tiles_y), block(RIGID_LANES, RIGID_WAVES);
  mc_pick(fa.w.pixel_spacing == 1.0f, [&](auto U) {
    mc_pick_outputs(fa.w.out_frames != nullptr, fa.w.out_sum != nullptr, [&](auto F, auto S) {
      hipLaunchKernelGGL((warp_field2<F.value, S.value, U.value>), grid, block, (size_t)GW_QUADS_PAD * 16, s, fa);
    });
  });
}
