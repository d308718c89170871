// The production deformation-field warp: bicubic frame resample along a cubic-spline shift lattice
// (+ optional fused frame sum) for fp32, fp16 and raw u8 / i16 frames -- warp_field_plan, warp_field3 and
// warp_field_slow -- and the entry points mc_warp_frames_*, which pick a route (field_route below).  The
// lattice tables come from field_tables.hip, the two fallback kernels live in warp_field_fallback.hip.
//
// No FMA contraction in this object: warp_field_common.h says why.
#include "warp_field_common.h"
#pragma clang fp contract(off)

// Measured setting (DESIGN.md section 4 has the alternatives)
#define GW3_ILP 1   // warp_field3: pixels of a lane in flight together (interior tile-frames); 1, 2 and 4 measure the same

// ------------------------------------------------------------------ warp_field3: 16 waves, double-buffered window
// What the counters said about one window per 4-wave workgroup (warp_field2; 40 x 4092 x 5760, sum only,
// 3.0 ms): 88 VALU instructions per pixel, almost all on the 2-cycle pipe, i.e. 1.1 ms of issue -- but a wave
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

// ------------------------------------------------------------------ host side
// Route rules.  The tile kernels DMA rows of whole 16-byte units (`unit` samples: fp32 4, fp16 / i16 8,
// u8 16) from an aligned stack ...
static bool field_whole_units(int w, uintptr_t frames, int unit) { return (w % unit) == 0 && (frames & 15) == 0; }
// ... warp_field3 stages <= GW3_EROWS lattice rows per tile: 32 pixel rows must span <= 1.5 lattice cells
// (always for the reference's 10 nodes per patch; not for a per-pixel lattice) ...
static bool field3_lattice_ok(int h, int GH) { return (int64_t)32 * (GH - 1) * 2 <= (int64_t)3 * (h - 1); }
// ... and it addresses a frame with 32-bit element offsets built by 24-bit multiplies
static bool field3_small32(int h, int w) { return h < (1 << 24) && w < (1 << 24) && (int64_t)h * w < ((int64_t)1 << 31); }

// The one route rule of the field warp.  Only fp32 frames have fallbacks: warp_main for other rows or
// stacks, warp_field2 for what warp_field3 cannot stage or address.  tests/field_reference.py::route_of
// restates the rule for the tests.
enum FieldRoute { ROUTE_MAIN, ROUTE_FIELD2, ROUTE_FIELD3, ROUTE_UNSUPPORTED };
static FieldRoute field_route(int storage, int h, int w, int GH, uintptr_t frames, int unit) {
  const bool f32 = storage == MC_STORE_F32;
  if (!field_whole_units(w, frames, unit)) return f32 ? ROUTE_MAIN : ROUTE_UNSUPPORTED;
  if (field3_lattice_ok(h, GH) && field3_small32(h, w)) return ROUTE_FIELD3;
  return f32 ? ROUTE_FIELD2 : ROUTE_UNSUPPORTED;
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
  const int unit = storage == MC_STORE_U8 ? 16 : 8;
  if (field_route(storage, h, w, GH, (uintptr_t)raw, unit) != ROUTE_FIELD3 || (((uintptr_t)gain) & 3)) return MC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const FieldScratch t = field_scratch(scratch, nframes, h, w, GH);
  mc_field_tables_launch(lattice, nframes, h, w, GH, GW, t, s);
  const FieldArgs fa = field_args(raw, nframes, h, w, lattice, GH, GW, pixel_spacing, t, out_frames, out_sum, gain, mu);
  hipError_t e = hipMemsetAsync(t.flags, 0, (size_t)t.flag_bytes, s);
  if (e != hipSuccess) return (int)e;
  if (storage == MC_STORE_U8) field3_launch<1>(fa, t, false, accumulate, s);
  else field3_launch<2>(fa, t, false, accumulate, s);
  return mc_check_launch();
}

extern "C" {

int mc_warp_frames_t(const void* frames, int storage, int nframes, int h, int w, const float* lattice,
                     int GH, int GW, float pixel_spacing, float* scratch, float* out_frames, float* out_sum,
                     void* stream) {
  if (storage != MC_STORE_F32 && storage != MC_STORE_F16) return MC_ERR_UNSUPPORTED;
  const bool half = storage == MC_STORE_F16;
  const int unit = half ? 8 : 4;
  // fp16 frames take warp_field3 only: 16-byte rows of 8 samples and the reference's sparse lattice (10
  // nodes per patch).  Those shapes are refused before the arguments are looked at (callers probe with the
  // shape alone, then widen the stack); a frame beyond 32-bit offsets is refused after them, by the route.
  if (half && !(field_whole_units(w, (uintptr_t)frames, unit) && field3_lattice_ok(h, GH))) return MC_ERR_UNSUPPORTED;
  if (!frames || !lattice || !scratch || (!out_frames && !out_sum)) return MC_ERR_ARG;
  if (nframes < 1 || h < 2 || w < 2 || GH < 1 || GW < 1 || !(pixel_spacing > 0.f)) return MC_ERR_ARG;
  if (((uintptr_t)scratch) & 15) return MC_ERR_ARG;
  // an fp16 stack never reaches a fallback: they read fp32 only, twice the buffer's bytes
  const FieldRoute route = field_route(storage, h, w, GH, (uintptr_t)frames, unit);
  if (route == ROUTE_UNSUPPORTED) return MC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const FieldScratch t = field_scratch(scratch, nframes, h, w, GH);
  mc_field_tables_launch(lattice, nframes, h, w, GH, GW, t, s);
  const FieldArgs fa = field_args(frames, nframes, h, w, lattice, GH, GW, pixel_spacing, t, out_frames, out_sum, nullptr, nullptr);
  if (route == ROUTE_MAIN) {
    mc_warp_main_launch(fa.w, s);
    return mc_check_launch();
  }
  hipError_t e = hipMemsetAsync(t.flags, 0, (size_t)t.flag_bytes, s);
  if (e != hipSuccess) return (int)e;
  if (route == ROUTE_FIELD3) {
    field3_launch<0>(fa, t, half, false, s);
  } else {
    mc_warp_field2_launch(fa, s);
    mc_pick(pixel_spacing == 1.0f, [&](auto U) { field_slow_launch<U.value, false, 0>(fa, s); });
  }
  return mc_check_launch();
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

}  // extern "C"
