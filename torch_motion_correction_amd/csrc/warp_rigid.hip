// Rigid (whole-frame shift) warp of fp32 and fp16 frames, and the weight tables every rigid kernel reads
// (warp_rigid_raw.hip gets them through mc_rigid_tables_launch).
//
// A (2,nt,1,1) field gives every frame one shift (sy, sx) [px].  The coordinate chain
// of sample_image_2d then depends on y alone (rows) and x alone (columns), so the
// bicubic resample is a separable correlation whose 4 taps per axis sit at
// floor(u)-1..floor(u)+2.  floor(u(p)) - p takes at most two adjacent values along an
// axis (u = p + s up to fp32 rounding), so with S = min(floor(u(p)) - p) every output
// uses the 5 input samples p+S-1 .. p+S+3 with the 4 weights placed at offset
// d = floor(u(p)) - p - S in {0,1} (the fifth weight is an exact zero): same products,
// same summation order as the 4-tap form, but a perfectly regular access pattern.
// Rows/columns whose coordinate leaves [0,n-1] get all-zero weights (the reference
// zeroes those samples).  The reference's own per-pixel shift is the bicubic upsample
// of a constant lattice, i.e. s*(1 +- ~2e-6); here s is used as is.
//
// The resampling kernels may contract to FMA, so that is the file's mode; the three table kernels carry
// the strict fp32 coordinate chain and switch contraction off in their own bodies.
#include "warp_common.h"
#include "mcorr.h"
#pragma clang fp contract(fast)

// Measured settings (DESIGN.md section 4 has the alternatives, none faster)
#define RIGID_MINW 2       // warp_rigid: workgroups per CU the register budget is held to
#define RIGID_SB 2         // strip bodies: window rows of LDS reads in flight between scheduling barriers
#define RIGID_DMA_WX 2     // warp_rigid_dma / warp_rigid_dma_h tile: 2 waves side by side (256 columns each)
#define RIGID_DMA_WY 4     //   x 4 waves down (8 rows each) = 512 x 32 output pixels per workgroup
#define RIGID_DMA_MINW 4   // 16 waves per CU
#define RIGID_TROWS (RIGID_WAVES * RIGID_ROWS + 4)     // input rows per tile (36)
#define RIGID_QUADS (RIGID_LANES + 4)                  // float4 columns per tile row (68)
#define RIGID_PLANE (RIGID_QUADS + 1)                  // plane stride in floats (odd: no conflicts)
#define RIGID_RSTRIDE (4 * RIGID_PLANE)                // LDS floats per tile row
#define RIGID_NQ (RIGID_TROWS * RIGID_QUADS)           // quads per tile (2448)
#define RIGID_QPT ((RIGID_NQ + 255) / 256)             // quads per thread (10)

// This thread's share of min_p floor(u(p)) - p over an axis of n samples shifted by s (256 threads).  The
// shuffle tree and part[4] stay written out in rigid_base and rigid_tail: inside this helper, in any form,
// they changed both kernels' code.
__device__ __forceinline__ int rigid_min_offset(float s, int n) {
#pragma clang fp contract(off)
  // clamp the (finite) offset so absurd shifts cannot overflow
  const float lim = 3.0f * (float)n + 16.f;
  int di = 0x7fffffff;
  for (int p = threadIdx.x; p < n; p += 256) {
    const float u = grid_chain((float)p + s, (float)n);
    const float d = floorf(u) - (float)p;
    di = min(di, (int)fminf(fmaxf(d, -lim), lim));
  }
  return di;
}

// pass 0: S[f][axis] = min_p floor(u(p)) - p.  One workgroup per (frame, axis): no atomics,
// no pre-set of S (80 words fought over by 1280 workgroups cost 20 us in atomics alone).
__global__ __launch_bounds__(256) void rigid_base(const float* __restrict__ shifts, int nframes, int h,
                                                  int w, int* __restrict__ S) {
#pragma clang fp contract(off)
  const int f = blockIdx.x, axis = blockIdx.y;
  const int n = axis == 0 ? h : w;
  int di = rigid_min_offset(shifts[2 * f + axis], n);
  for (int off = 32; off > 0; off >>= 1) di = min(di, __shfl_xor(di, off));
  __shared__ int part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = di;
  __syncthreads();
  if (threadIdx.x == 0) S[2 * f + axis] = min(min(part[0], part[1]), min(part[2], part[3]));
}

// pass 1: W[f][axis][k][p], k = 0..4
__global__ void rigid_weights(const float* __restrict__ shifts, int nframes, int h, int w,
                              const int* __restrict__ S, float* __restrict__ Wy,
                              float* __restrict__ Wx) {
#pragma clang fp contract(off)
  const int f = blockIdx.y, axis = blockIdx.z;
  const int n = axis == 0 ? h : w;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const float s = shifts[2 * f + axis];
  const float c = (float)p + s;
  const bool inside = (c >= 0.f) && (c <= (float)n - 1.f);
  const float u = grid_chain(c, (float)n);
  const float fl = floorf(u);
  float wt[4];
  cubic_coeffs_fast(u - fl, wt);
  const float lim = 3.0f * (float)n + 16.f;
  const int d = (int)fminf(fmaxf(fl - (float)p, -lim), lim) - S[2 * f + axis];
  float out[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (inside && d >= 0 && d <= 1) {
    for (int k = 0; k < 4; ++k) out[k + d] = wt[k];
  }
  if (axis == 0) {
    float* W = Wy + ((int64_t)f * n + p) * 5;  // [f][y][5]: a strip's weights are contiguous
    for (int k = 0; k < 5; ++k) W[k] = out[k];
  } else {
    float* W = Wx + (int64_t)f * 5 * n;  // [f][5][x]: float4 per tap for 4 adjacent columns
    for (int k = 0; k < 5; ++k) W[(int64_t)k * n + p] = out[k];
  }
}

// pass 0 for the movie pipeline, everything between the peak search and the weight tables in ONE launch:
// the pipeline's tail used to be six launches of a few microseconds each (shifts * pixel_spacing, a
// contiguous copy, spline_lattice_kernel, another copy, / pixel_spacing, rigid_base), all on the
// estimator's critical chain and each waiting for a wave slot under the previous movie's warp.  One
// workgroup per (frame, axis): the frame's lattice value = the (2,t,1,1) field's spline in time at
// t_f = f / (t - 1) -- spline_lattice_kernel's arithmetic in spline_lattice_kernel's order, lattice point
// (0, 0), so the result is bit for bit what the generic route gives --, then rigid_base's reduction.
//   field[axis][f] = shifts[f][axis] * ps;  shifts_px[f][axis] = lattice / ps;  S[f][axis] as rigid_base
__global__ __launch_bounds__(256) void rigid_tail(const float* __restrict__ shifts, float ps, const int* __restrict__ idx_t,
                                                  const float* __restrict__ w_t, const float* __restrict__ w_y,
                                                  const float* __restrict__ w_x, int nframes, int h, int w,
                                                  float* __restrict__ field, float* __restrict__ shifts_px,
                                                  int* __restrict__ S) {
#pragma clang fp contract(off)
  const int f = blockIdx.x, axis = blockIdx.y;
  float vt = 0.f;
  for (int kt = 0; kt < 4; ++kt) {
    const float d = shifts[2 * idx_t[4 * f + kt] + axis] * ps;  // the field's node value (deformation_field_utils.py:129-162)
    float vy = 0.f;
    for (int ky = 0; ky < 4; ++ky) {
      float vx = 0.f;
      for (int kx = 0; kx < 4; ++kx) vx += d * w_x[kx];
      vy += vx * w_y[ky];
    }
    vt += vy * w_t[4 * f + kt];
  }
  const float s = vt / ps;
  if (threadIdx.x == 0) {
    field[axis * nframes + f] = shifts[2 * f + axis] * ps;
    shifts_px[2 * f + axis] = s;
  }
  const int n = axis == 0 ? h : w;
  int di = rigid_min_offset(s, n);
  for (int off = 32; off > 0; off >>= 1) di = min(di, __shfl_xor(di, off));
  __shared__ int part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = di;
  __syncthreads();
  if (threadIdx.x == 0) S[2 * f + axis] = min(min(part[0], part[1]), min(part[2], part[3]));
}

// Workgroup = 4 waves = tile of 256 x 32 output pixels.  Per frame the tile's 36 x 272
// input window (row/column indices clipped to the image = border padding) is fetched
// ONCE with 16-byte loads and parked in LDS de-interleaved by (column mod 4): the
// window is misaligned by m = (x_tile + Sx - 1) mod 4 floats, and with four planes lane l
// reads tap j at plane (m+j)&3, index l + ((m+j)>>2): consecutive lanes, consecutive
// banks.  Loads for frame f+1 are in flight (registers) while frame f is computed.
template <bool WRITE_FRAMES, bool WRITE_SUM>
__global__ __launch_bounds__(RIGID_LANES* RIGID_WAVES, RIGID_MINW) void warp_rigid(RigidArgs a) {
  __shared__ float tileS[RIGID_TROWS * RIGID_RSTRIDE];
  const int nt = a.tiles_x * a.tiles_y;
  const int b = blockIdx.x;
  int tile = b;
  if ((nt & 7) == 0) tile = (b & 7) * (nt >> 3) + (b >> 3);  // one band of tile rows per XCD
  const int tyi = tile / a.tiles_x, txi = tile - tyi * a.tiles_x;
  const int h = a.h, w = a.w;
  const int lane = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int tid = wave * RIGID_LANES + lane;
  const int xt = txi * (RIGID_LANES * 4);
  const int yt = tyi * (RIGID_WAVES * RIGID_ROWS);
  const int x0 = xt + lane * 4;
  const int y0 = yt + wave * RIGID_ROWS;
  const int64_t hw = (int64_t)h * w;
  const bool full = (x0 + 4 <= w) && ((w & 3) == 0);
  const bool wq = ((w & 3) == 0);
  float acc[RIGID_ROWS][4];
#pragma unroll
  for (int r = 0; r < RIGID_ROWS; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[r][k] = 0.f;

  const int f_lo = a.frames_in_grid ? (int)blockIdx.y * a.frames_in_grid : 0;
  const int f_hi = a.frames_in_grid ? min(f_lo + a.frames_in_grid, a.nframes) : a.nframes;

  float4 pre[RIGID_QPT];
  auto fetch = [&](int f) {  // issue the tile loads of frame f into `pre`
    const float* fr = a.frames + (int64_t)f * hw;
    const int Sy = a.S[2 * f], Sx = a.S[2 * f + 1];
    const int cxt = xt + Sx - 1;
    const int ax = cxt & ~3;  // aligned-down first column (two's complement: works for cxt < 0)
    const bool fast = wq && ax >= 0 && ax + 4 * RIGID_QUADS <= w;
#pragma unroll
    for (int i = 0; i < RIGID_QPT; ++i) {
      const int q = tid + i * 256;
      if (q < RIGID_NQ) {
        const int tr = q / RIGID_QUADS, qc = q - tr * RIGID_QUADS;
        int r = yt + Sy - 1 + tr;
        r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
        const float* row = fr + (int64_t)r * w;
        const int c = ax + 4 * qc;
        if (fast) {
          pre[i] = *reinterpret_cast<const float4*>(row + c);
        } else {
          float e[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            int cc = c + k;
            cc = cc < 0 ? 0 : (cc > w - 1 ? w - 1 : cc);
            e[k] = row[cc];
          }
          pre[i] = make_float4(e[0], e[1], e[2], e[3]);
        }
      }
    }
  };
  auto park = [&]() {  // registers -> LDS planes
#pragma unroll
    for (int i = 0; i < RIGID_QPT; ++i) {
      const int q = tid + i * 256;
      if (q < RIGID_NQ) {
        const int tr = q / RIGID_QUADS, qc = q - tr * RIGID_QUADS;
        float* d = tileS + tr * RIGID_RSTRIDE + qc;
        d[0] = pre[i].x;
        d[RIGID_PLANE] = pre[i].y;
        d[2 * RIGID_PLANE] = pre[i].z;
        d[3 * RIGID_PLANE] = pre[i].w;
      }
    }
  };

  fetch(f_lo);
  park();
  __syncthreads();
  for (int f = f_lo; f < f_hi; ++f) {
    if (f + 1 < f_hi) fetch(f + 1);
    const int Sx = a.S[2 * f + 1];
    const int m = (xt + Sx - 1) & 3;
    // row weights of this wave's strip: Wy[f][y][5] -> 40 consecutive floats, one per lane
    float wyv = 0.f;
    {
      const int64_t idx = (int64_t)y0 * 5 + lane;
      if (lane < 5 * RIGID_ROWS && idx < (int64_t)h * 5) wyv = a.Wy[(int64_t)f * 5 * h + idx];
    }
    float wx[5][4];
    const float* Wx = a.Wx + (int64_t)f * 5 * w + x0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      if (full) {
        const float4 t = *reinterpret_cast<const float4*>(Wx + (int64_t)j * w);
        wx[j][0] = t.x; wx[j][1] = t.y; wx[j][2] = t.z; wx[j][3] = t.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) wx[j][k] = (x0 + k < w) ? Wx[(int64_t)j * w + k] : 0.f;
      }
    }
    // per-tap LDS offsets (wave-uniform): plane (m+j)&3, index lane + ((m+j)>>2)
    int toff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) toff[j] = ((m + j) & 3) * RIGID_PLANE + ((m + j) >> 2);
    const float* wrow = tileS + (wave * RIGID_ROWS) * RIGID_RSTRIDE + lane;
    float H[5][4];
#pragma unroll
    for (int rr = 0; rr < RIGID_ROWS + 4; ++rr) {
      // keep at most two rows of LDS reads in flight: without this the scheduler hoists
      // all 96 reads and the kernel needs > 240 VGPRs
      if ((rr % RIGID_SB) == 0) __builtin_amdgcn_sched_barrier(0);
      const float* src = wrow + rr * RIGID_RSTRIDE;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[toff[j]];
      float* Hn = H[rr % 5];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        Hn[k] = (((wx[0][k] * v[k] + wx[1][k] * v[k + 1]) + wx[2][k] * v[k + 2]) +
                 wx[3][k] * v[k + 3]) + wx[4][k] * v[k + 4];
      if (rr >= 4) {
        const int ro = rr - 4;
        const int yo = y0 + ro;
        float wy[5];
#pragma unroll
        for (int i = 0; i < 5; ++i)
          wy[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wyv), ro * 5 + i));
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          o[k] = (((wy[0] * H[(ro + 0) % 5][k] + wy[1] * H[(ro + 1) % 5][k]) +
                   wy[2] * H[(ro + 2) % 5][k]) + wy[3] * H[(ro + 3) % 5][k]) +
                 wy[4] * H[(ro + 4) % 5][k];
        if (yo < h && x0 < w) {
          if (WRITE_FRAMES) {
            float* dst = a.out_frames + (int64_t)f * hw + (int64_t)yo * w + x0;
            if (full) {
              *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
              for (int k = 0; k < 4 && x0 + k < w; ++k) dst[k] = o[k];
            }
          }
          if (WRITE_SUM) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[ro][k] += o[k];
          }
        }
      }
    }
    __syncthreads();  // everyone is done reading the tile of frame f
    if (f + 1 < f_hi) {
      park();
      __syncthreads();
    }
  }
  if (WRITE_SUM && x0 < w) {
#pragma unroll
    for (int ro = 0; ro < RIGID_ROWS; ++ro) {
      const int yo = y0 + ro;
      if (yo < h) {
        float* dst = a.out_sum + (int64_t)yo * w + x0;
        for (int k = 0; k < 4 && x0 + k < w; ++k) dst[k] = acc[ro][k];  // one block owns the tile's sum
      }
    }
  }
}

// ------------------------------------------------------------------ rigid warp, LDS-DMA
// Same mathematics as warp_rigid; the 36 x 272 input window of a tile goes HBM -> LDS by
// `global_load_lds_dwordx4` (no VGPR staging, row-major image).  The global side of that
// DMA only needs 4-byte alignment, so the window starts exactly at column x_tile + Sx - 1:
// a lane's 8-float window is two aligned 16-byte LDS reads whatever the shift, and there
// is ONE strip body (four misalignment specialisations of it were 24 KB of straight-line
// code, which thrashed the instruction cache once blocks of different frames shared a CU,
// and cost 16 more VGPRs: the fused-sum kernel now fits 4 workgroups per CU).
// Single buffer, 4 workgroups per CU cover each other's DMA latency; double-buffering inside the
// workgroup was measured slower.  Columns outside the image (border padding =
// clipped tap coordinate) are re-fetched element-wise for edge tiles only.
// Requires w % 4 == 0 and 16-byte aligned frames (host checks; else warp_rigid).
#define RD_QUADS (RIGID_DMA_WX * RIGID_LANES + 4)  // float4 columns per tile row

// a0 b0 + a1 b1 + ... + a4 b4 as one product and four fused multiply-adds in this order: the fp32 and
// the fp16 strip bodies then round identically (left to the contraction pass the two bodies fused
// different products and differed in the last bit for 5 % of the pixels)
__device__ __forceinline__ float rigid_dot5(float a0, float b0, float a1, float b1, float a2, float b2, float a3,
                                            float b3, float a4, float b4) {
  float r = a0 * b0;
  r = __builtin_fmaf(a1, b1, r);
  r = __builtin_fmaf(a2, b2, r);
  r = __builtin_fmaf(a3, b3, r);
  return __builtin_fmaf(a4, b4, r);
}

#define RDH_QH (RIGID_DMA_WX * 32 + 1)  // 16-byte units (8 samples) per tile row
__device__ __forceinline__ float rh_lo(unsigned v) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)(v & 0xffffu));
}
__device__ __forceinline__ float rh_hi(unsigned v) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(v >> 16)); }


// How window row rr in LDS becomes the lane's 8 samples e[0..7]: all that the two storages' strips differ in
struct RowF32 {
  const float4* wrow;  // the lane's first quad
  __device__ __forceinline__ void operator()(int rr, float (&e)[8]) const {
    const float4 q0 = wrow[rr * RD_QUADS], q1 = wrow[rr * RD_QUADS + 1];
    e[0] = q0.x; e[1] = q0.y; e[2] = q0.z; e[3] = q0.w;
    e[4] = q1.x; e[5] = q1.y; e[6] = q1.z; e[7] = q1.w;
  }
};
template <int P>  // parity of the window's first column
struct RowHalf {
  const uint2* wrow;  // the lane's first 8-byte unit (4 samples)
  __device__ __forceinline__ void operator()(int rr, float (&e)[8]) const {
    constexpr int UNITS8 = 2 * RDH_QH;  // 8-byte units per tile row
    const uint2 u0 = wrow[rr * UNITS8], u1 = wrow[rr * UNITS8 + 1];
    if constexpr (P == 0) {
      e[0] = rh_lo(u0.x); e[1] = rh_hi(u0.x); e[2] = rh_lo(u0.y); e[3] = rh_hi(u0.y);
      e[4] = rh_lo(u1.x); e[5] = rh_hi(u1.x); e[6] = rh_lo(u1.y); e[7] = rh_hi(u1.y);
    } else {
      const unsigned u2x = reinterpret_cast<const unsigned*>(wrow + rr * UNITS8 + 2)[0];
      e[0] = rh_hi(u0.x); e[1] = rh_lo(u0.y); e[2] = rh_hi(u0.y); e[3] = rh_lo(u1.x);
      e[4] = rh_hi(u1.x); e[5] = rh_lo(u1.y); e[6] = rh_hi(u1.y); e[7] = rh_lo(u2x);
    }
  }
};

// NT: frames leave by rigid_store4 (non-temporal; the fp32 kernel, measured there), else by a plain 16-byte store
template <bool WRITE_FRAMES, bool WRITE_SUM, bool FULL, bool NT, class Row>
__device__ __forceinline__ void rigid_strip(const RigidArgs& a, const Row row, int f, int y0, int x0, float wyv,
                                            const float (&wx)[5][4], float (&acc)[RIGID_ROWS][4]) {
  const int h = a.h, w = a.w;
  // FULL: the whole tile lies inside the image -> no per-row predicates, the strip is
  // one basic block and the scheduler can run the LDS reads ahead of the arithmetic
  float* orow = WRITE_FRAMES ? a.out_frames + (int64_t)f * h * w + (int64_t)y0 * w + x0 : nullptr;
  float H[5][4];
#pragma unroll
  for (int rr = 0; rr < RIGID_ROWS + 4; ++rr) {
    if ((rr % RIGID_SB) == 0) __builtin_amdgcn_sched_barrier(0);
    float e[8];
    row(rr, e);
    float* Hn = H[rr % 5];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      Hn[k] = rigid_dot5(wx[0][k], e[k], wx[1][k], e[k + 1], wx[2][k], e[k + 2], wx[3][k], e[k + 3], wx[4][k], e[k + 4]);
    if (rr >= 4) {
      const int ro = rr - 4;
      float wy[5];
#pragma unroll
      for (int i = 0; i < 5; ++i)
        wy[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wyv), ro * 5 + i));
      float o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        o[k] = rigid_dot5(wy[0], H[(ro + 0) % 5][k], wy[1], H[(ro + 1) % 5][k], wy[2], H[(ro + 2) % 5][k], wy[3],
                          H[(ro + 3) % 5][k], wy[4], H[(ro + 4) % 5][k]);
      if (FULL || (y0 + ro < h && x0 < w)) {
        if (WRITE_FRAMES) {
          if (NT) rigid_store4(orow + (int64_t)ro * w, o[0], o[1], o[2], o[3]);
          else *reinterpret_cast<float4*>(orow + (int64_t)ro * w) = make_float4(o[0], o[1], o[2], o[3]);
        }
        if (WRITE_SUM) {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[ro][k] += o[k];
        }
      }
    }
  }
}

// The 512 x 32 tile (against the 256 x 32 one of warp_rigid) makes every row piece a workgroup touches
// longer: fewer partial 128-byte lines at the two ends, longer runs inside a DRAM page.
template <bool WRITE_FRAMES, bool WRITE_SUM>
__global__ __launch_bounds__(RIGID_LANES* RIGID_DMA_WX* RIGID_DMA_WY, RIGID_DMA_MINW)
void warp_rigid_dma(RigidArgs a) {
  constexpr int WX = RIGID_DMA_WX, WY = RIGID_DMA_WY, NWAVES = WX * WY;
  constexpr int TROWS = WY * RIGID_ROWS + 4;       // input rows per tile
  constexpr int QUADS = RD_QUADS;
  constexpr int NQ = TROWS * QUADS;
  constexpr int QUADS_PAD = ((NQ + 63) / 64) * 64;  // DMA granule: 64 lanes x 16 B
  extern __shared__ __attribute__((aligned(16))) char smem_rd[];
  float4* const b0 = reinterpret_cast<float4*>(smem_rd);
  const int nt = a.tiles_x * a.tiles_y;
  const int b = blockIdx.x;
  int tile = b;
  if ((nt & 7) == 0) tile = (b & 7) * (nt >> 3) + (b >> 3);  // one band of tile rows per XCD
  const int tyi = tile / a.tiles_x, txi = tile - tyi * a.tiles_x;
  const int h = a.h, w = a.w;
  const int lane = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int wvx = wave % WX, wvy = wave / WX;
  const int tid = wave * RIGID_LANES + lane;
  const int xt = txi * (RIGID_LANES * 4 * WX);
  const int yt = tyi * (WY * RIGID_ROWS);
  const int x0 = xt + wvx * (RIGID_LANES * 4) + lane * 4;
  const int y0 = yt + wvy * RIGID_ROWS;
  const int64_t hw = (int64_t)h * w;
  float acc[RIGID_ROWS][4];
#pragma unroll
  for (int r = 0; r < RIGID_ROWS; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[r][k] = 0.f;
  const bool full_tile = yt + WY * RIGID_ROWS <= h && xt + RIGID_LANES * 4 * WX <= w;
  const int f_lo = a.frames_in_grid ? (int)blockIdx.y * a.frames_in_grid : 0;
  const int f_hi = a.frames_in_grid ? min(f_lo + a.frames_in_grid, a.nframes) : a.nframes;

  // DMA of one frame's window into `dst`: granule i = quads [64 i, 64 i + 64)
  auto dma = [&](int f, float4* dst) {
    const float* fr = a.frames + (int64_t)f * hw;
    const int Sy = a.S[2 * f], Sx = a.S[2 * f + 1];
    const int ax = xt + Sx - 1;  // any multiple of 4 BYTES: the global side of the DMA needs no more
    for (int i = wave; i < QUADS_PAD / 64; i += NWAVES) {
      int q = i * 64 + lane;
      q = q < NQ ? q : NQ - 1;  // tail lanes re-load the last quad into the pad
      const int tr = q / QUADS, qc = q - tr * QUADS;
      int r = yt + Sy - 1 + tr;
      r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
      int c = ax + 4 * qc;
      c = c < 0 ? 0 : (c > w - 4 ? w - 4 : c);  // whole quads inside the row; clamped ones are patched
      __builtin_amdgcn_global_load_lds(fr + (int64_t)r * w + c, (lds_vptr)(dst + i * 64), 16, 0, 0);
    }
  };
  // border padding for edge tiles: a quad whose 4 columns are not all inside the row was
  // DMA'd from a clamped address and holds the wrong columns; its elements are re-fetched
  // one by one at their clipped column (a handful of quads per row, edge tiles only)
  auto patch = [&](int f, float4* t4) {
    const int Sy = a.S[2 * f], Sx = a.S[2 * f + 1];
    const int ax = xt + Sx - 1;
    if (ax >= 0 && ax + 4 * QUADS <= w) return false;
    const float* fr = a.frames + (int64_t)f * hw;
    float* t = reinterpret_cast<float*>(t4);
    for (int q = tid; q < NQ; q += RIGID_LANES * NWAVES) {
      const int tr = q / QUADS, qc = q - tr * QUADS;
      const int s0 = ax + 4 * qc;
      if (s0 >= 0 && s0 <= w - 4) continue;
      int r = yt + Sy - 1 + tr;
      r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int c = s0 + e;
        c = c < 0 ? 0 : (c > w - 1 ? w - 1 : c);
        t[4 * q + e] = fr[(int64_t)r * w + c];
      }
    }
    return true;
  };

  float wx[5][4];
  float wyv = 0.f;
  const int strip = (wvy * RIGID_ROWS) * QUADS + wvx * RIGID_LANES + lane;  // this lane's first quad

  rigid_load_weights(a, f_lo, y0, x0, lane, wx, wyv);
  dma(f_lo, b0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (patch(f_lo, b0)) __syncthreads();
  for (int f = f_lo; f < f_hi; ++f) {
    const float4* t = b0 + strip;
    if (full_tile) rigid_strip<WRITE_FRAMES, WRITE_SUM, true, true>(a, RowF32{t}, f, y0, x0, wyv, wx, acc);
    else rigid_strip<WRITE_FRAMES, WRITE_SUM, false, true>(a, RowF32{t}, f, y0, x0, wyv, wx, acc);
    if (f + 1 < f_hi) {
      // single buffer, several workgroups per CU: other workgroups cover this one's latency,
      // so nothing is double-buffered here (registers are the scarce resource)
      __syncthreads();  // everyone must be done reading before the tile is refilled
      dma(f + 1, b0);
      rigid_load_weights(a, f + 1, y0, x0, lane, wx, wyv);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (patch(f + 1, b0)) __syncthreads();
    }
  }
  if (WRITE_SUM && x0 < w) {
#pragma unroll
    for (int ro = 0; ro < RIGID_ROWS; ++ro) {
      const int yo = y0 + ro;
      if (yo < h) {
        // one block owns its tile's sum over all frames: a plain store (no zero fill, no read-back);
        // w % 4 == 0 on this path, so the quad is 16-byte aligned whenever out_sum is
        float* dst = a.out_sum + (int64_t)yo * w + x0;
        if ((((uintptr_t)a.out_sum) & 15) == 0) {
          *reinterpret_cast<float4*>(dst) = make_float4(acc[ro][0], acc[ro][1], acc[ro][2], acc[ro][3]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) dst[k] = acc[ro][k];
        }
      }
    }
  }
}

// ------------------------------------------------------------------ rigid warp, LDS-DMA, fp16 frames
// The same kernel for frames stored as fp16 (N2: fp16 storage read natively): the window goes
// HBM -> LDS as the raw 16-bit samples -- half the bytes of the fp32 kernel on the read side -- and is
// widened on the way from LDS to the registers (8 v_cvt_f32_f16 per window row of a lane).  The
// global side of the DMA needs 4-byte alignment, so the window starts at the EVEN column at or left
// of x_tile + Sx - 1; the parity p of that column is wave-uniform per frame and selects one of two
// strip bodies with compile-time sample positions: a lane's 8-sample window is the halfs
// [4 L + p, 4 L + p + 8) of the tile row = two (p = 0) or three (p = 1) aligned ds_read_b64.
// Tile rows hold RDH_QH = 32 RIGID_DMA_WX + 1 units of 8 samples.  Requires w % 8 == 0 and 16-byte aligned frames.
template <bool WRITE_FRAMES, bool WRITE_SUM>
__global__ __launch_bounds__(RIGID_LANES* RIGID_DMA_WX* RIGID_DMA_WY, RIGID_DMA_MINW)
void warp_rigid_dma_h(RigidArgs a) {
  constexpr int WX = RIGID_DMA_WX, WY = RIGID_DMA_WY, NWAVES = WX * WY;
  constexpr int TROWS = WY * RIGID_ROWS + 4;   // input rows per tile
  constexpr int QH = RDH_QH;
  constexpr int NQ = TROWS * QH;
  constexpr int UNITS_PAD = ((NQ + 63) / 64) * 64;  // DMA granule: 64 lanes x 16 B
  extern __shared__ __attribute__((aligned(16))) char smem_rd[];
  float4* const b0 = reinterpret_cast<float4*>(smem_rd);
  const _Float16* const frames = reinterpret_cast<const _Float16*>(a.frames);
  const int nt = a.tiles_x * a.tiles_y;
  const int b = blockIdx.x;
  int tile = b;
  if ((nt & 7) == 0) tile = (b & 7) * (nt >> 3) + (b >> 3);  // one band of tile rows per XCD
  const int tyi = tile / a.tiles_x, txi = tile - tyi * a.tiles_x;
  const int h = a.h, w = a.w;
  const int lane = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int wvx = wave % WX, wvy = wave / WX;
  const int tid = wave * RIGID_LANES + lane;
  const int xt = txi * (RIGID_LANES * 4 * WX);
  const int yt = tyi * (WY * RIGID_ROWS);
  const int x0 = xt + wvx * (RIGID_LANES * 4) + lane * 4;
  const int y0 = yt + wvy * RIGID_ROWS;
  const int64_t hw = (int64_t)h * w;
  float acc[RIGID_ROWS][4];
#pragma unroll
  for (int r = 0; r < RIGID_ROWS; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[r][k] = 0.f;
  const bool full_tile = yt + WY * RIGID_ROWS <= h && xt + RIGID_LANES * 4 * WX <= w;
  const int f_lo = a.frames_in_grid ? (int)blockIdx.y * a.frames_in_grid : 0;
  const int f_hi = a.frames_in_grid ? min(f_lo + a.frames_in_grid, a.nframes) : a.nframes;

  auto dma = [&](int f) {
    const _Float16* fr = frames + (int64_t)f * hw;
    const int Sy = a.S[2 * f], Sx = a.S[2 * f + 1];
    const int axe = (xt + Sx - 1) & ~1;  // even column: 4-byte aligned on the global side
    for (int i = wave; i < UNITS_PAD / 64; i += NWAVES) {
      int q = i * 64 + lane;
      q = q < NQ ? q : NQ - 1;  // tail lanes re-load the last unit into the pad
      const int tr = q / QH, qc = q - tr * QH;
      int r = yt + Sy - 1 + tr;
      r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
      int c = axe + 8 * qc;
      c = c < 0 ? 0 : (c > w - 8 ? w - 8 : c);  // whole units inside the row; clamped ones are patched
      __builtin_amdgcn_global_load_lds(fr + (int64_t)r * w + c, (lds_vptr)(b0 + i * 64), 16, 0, 0);
    }
  };
  // border padding for edge tiles: a unit whose 8 columns are not all inside the row was DMA'd from a
  // clamped address; its samples are re-fetched one by one at their clipped column
  auto patch = [&](int f) {
    const int Sy = a.S[2 * f], Sx = a.S[2 * f + 1];
    const int axe = (xt + Sx - 1) & ~1;
    if (axe >= 0 && axe + 8 * QH <= w) return false;
    const _Float16* fr = frames + (int64_t)f * hw;
    _Float16* t = reinterpret_cast<_Float16*>(b0);
    for (int q = tid; q < NQ; q += RIGID_LANES * NWAVES) {
      const int tr = q / QH, qc = q - tr * QH;
      const int s0 = axe + 8 * qc;
      if (s0 >= 0 && s0 <= w - 8) continue;
      int r = yt + Sy - 1 + tr;
      r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int c = s0 + e;
        c = c < 0 ? 0 : (c > w - 1 ? w - 1 : c);
        t[8 * q + e] = fr[(int64_t)r * w + c];
      }
    }
    return true;
  };

  float wx[5][4];
  float wyv = 0.f;
  // rigid_load_weights, written out: the shared function changed three of this kernel's four instantiations
  auto load_weights = [&](int f) {
    wyv = 0.f;
    const int64_t idx = (int64_t)y0 * 5 + lane;
    if (lane < 5 * RIGID_ROWS && idx < (int64_t)h * 5) wyv = a.Wy[(int64_t)f * 5 * h + idx];
    const float* Wx = a.Wx + (int64_t)f * 5 * w + x0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (x0 < w) t = *reinterpret_cast<const float4*>(Wx + (int64_t)j * w);
      wx[j][0] = t.x; wx[j][1] = t.y; wx[j][2] = t.z; wx[j][3] = t.w;
    }
  };
  // this lane's first 8-byte unit (4 samples): row (wvy RIGID_ROWS), sample 4 (64 wvx + lane)
  const uint2* const strip = reinterpret_cast<const uint2*>(b0) + (wvy * RIGID_ROWS) * (2 * QH) + wvx * RIGID_LANES + lane;

  load_weights(f_lo);
  dma(f_lo);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (patch(f_lo)) __syncthreads();
  for (int f = f_lo; f < f_hi; ++f) {
    const int par = __builtin_amdgcn_readfirstlane((xt + a.S[2 * f + 1] - 1) & 1);
    if (par) {
      if (full_tile) rigid_strip<WRITE_FRAMES, WRITE_SUM, true, false>(a, RowHalf<1>{strip}, f, y0, x0, wyv, wx, acc);
      else rigid_strip<WRITE_FRAMES, WRITE_SUM, false, false>(a, RowHalf<1>{strip}, f, y0, x0, wyv, wx, acc);
    } else {
      if (full_tile) rigid_strip<WRITE_FRAMES, WRITE_SUM, true, false>(a, RowHalf<0>{strip}, f, y0, x0, wyv, wx, acc);
      else rigid_strip<WRITE_FRAMES, WRITE_SUM, false, false>(a, RowHalf<0>{strip}, f, y0, x0, wyv, wx, acc);
    }
    if (f + 1 < f_hi) {
      __syncthreads();  // everyone must be done reading before the tile is refilled
      dma(f + 1);
      load_weights(f + 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (patch(f + 1)) __syncthreads();
    }
  }
  if (WRITE_SUM && x0 < w) {
#pragma unroll
    for (int ro = 0; ro < RIGID_ROWS; ++ro) {
      const int yo = y0 + ro;
      if (yo < h) {
        float* dst = a.out_sum + (int64_t)yo * w + x0;
        if ((((uintptr_t)a.out_sum) & 15) == 0) {
          *reinterpret_cast<float4*>(dst) = make_float4(acc[ro][0], acc[ro][1], acc[ro][2], acc[ro][3]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) dst[k] = acc[ro][k];
        }
      }
    }
  }
}

void mc_rigid_tables_launch(const float* shifts_px, int nframes, int h, int w, const RigidTables& t, hipStream_t s) {
  const int n = h > w ? h : w;
  hipLaunchKernelGGL(rigid_base, dim3(nframes, 2), dim3(256), 0, s, shifts_px, nframes, h, w, t.S);
  hipLaunchKernelGGL(rigid_weights, dim3((n + 255) / 256, nframes, 2), dim3(256), 0, s, shifts_px, nframes, h, w,
                     (const int*)t.S, t.Wy, t.Wx);
}

extern "C" {

// phase: see rigid_check_args (warp_common.h)
int mc_warp_rigid_phase_t(const void* frames, int storage, int nframes, int h, int w, const float* shifts_px,
                          float* scratch, float* out_frames, float* out_sum, int phase, void* stream) {
  if (storage != MC_STORE_F32 && storage != MC_STORE_F16) return MC_ERR_UNSUPPORTED;
  // fp16 frames: only the LDS-DMA kernel's 512 x 32 geometry, rows of whole 8-sample units
  if (storage == MC_STORE_F16 && ((w % 8) != 0 || (((uintptr_t)frames) & 15) ||
                                  (out_frames && (((uintptr_t)out_frames) & 15))))
    return MC_ERR_UNSUPPORTED;
  if (const int e = rigid_check_args(frames, shifts_px, scratch, out_frames, out_sum, nframes, h, w, phase)) return e;
  hipStream_t s = (hipStream_t)stream;
  const RigidTables t = rigid_tables_layout(scratch, nframes, h, w);
  if (rigid_phase_tables(phase, shifts_px, nframes, h, w, t, s)) return mc_check_launch();
  // the LDS-DMA kernels' 512 x 32 tiles (fp16 frames have no other kernel), else warp_rigid's 256 x 32
  const bool half = storage == MC_STORE_F16;
  const bool dma_ok = half || ((w % 4 == 0) && ((((uintptr_t)frames) & 15) == 0) &&
                               (!out_frames || ((((uintptr_t)out_frames) & 15) == 0)));
  const int WX = dma_ok ? RIGID_DMA_WX : 1, WY = dma_ok ? RIGID_DMA_WY : RIGID_WAVES;
  // Without the fused sum every frame is its own block: blocks are dispatched frame-major, so the
  // resident ones always work on neighbouring tiles of ONE frame and halo rows / shared 128-byte
  // lines hit in L2 (FETCH_SIZE 2.76 GB for 2.68 GB of frames).  With the sum a block keeps its
  // tile's partial sums in registers over all frames; blocks drift apart in time and the same
  // halos miss (3.7 GB) -- measured 0.97 ms vs 1.28 ms at 40 x 4096^2.
  const RigidArgs a = rigid_args(frames, nframes, h, w, t, out_frames, out_sum, WX, WY, out_sum ? 0 : 1);
  const dim3 grid(a.tiles_x * a.tiles_y, a.frames_in_grid ? (nframes + a.frames_in_grid - 1) / a.frames_in_grid : 1),
      block(RIGID_LANES, WX * WY);
  mc_pick_outputs(out_frames != nullptr, out_sum != nullptr, [&](auto F, auto S) {
    if (!dma_ok) {
      hipLaunchKernelGGL((warp_rigid<F.value, S.value>), grid, block, 0, s, a);
      return;
    }
    // one tile's window: (RIGID_DMA_WY RIGID_ROWS + 4) rows of RD_QUADS float4 (fp16: RDH_QH units), whole wave-units
    const size_t lds = (size_t)((((RIGID_DMA_WY * RIGID_ROWS + 4) * (half ? RDH_QH : RD_QUADS)) + 63) / 64) * 64 * 16;
    auto k = half ? warp_rigid_dma_h<F.value, S.value> : warp_rigid_dma<F.value, S.value>;
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, grid, block, lds, s, a);
  });
  return mc_check_launch();
}

int mc_warp_rigid_scratch_bytes(int nframes, int h, int w, int64_t* bytes) {
  if (!bytes || nframes < 1 || h < 2 || w < 2) return MC_ERR_ARG;
  *bytes = rigid_tables_layout(nullptr, nframes, h, w).bytes;
  return MC_OK;
}

// The movie pipeline's tail in two launches (rigid_tail + rigid_weights): integer-peak shifts (t,2) px ->
// field (2,t) Angstrom, the warp's shifts_px (t,2) and its weight tables in `scratch` (the layout of
// mc_warp_rigid_phase_t, phase 1).  idx_t / w_t: the 4 time taps per frame of the field's spline
// (spline.axis_taps(t, linspace(0,1,t))), w_y / w_x: the taps of lattice point 0 on a 1-sample axis.
int mc_rigid_tables_from_shifts(const float* shifts, float pixel_spacing, const int* idx_t, const float* w_t,
                                const float* w_y, const float* w_x, int nframes, int h, int w, float* field,
                                float* shifts_px, float* scratch, void* stream) {
  if (!shifts || !idx_t || !w_t || !w_y || !w_x || !field || !shifts_px || !scratch) return MC_ERR_ARG;
  if (nframes < 1 || h < 2 || w < 2 || !(pixel_spacing > 0.f) || (((uintptr_t)scratch) & 15)) return MC_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const RigidTables t = rigid_tables_layout(scratch, nframes, h, w);
  const int n = h > w ? h : w;
  hipLaunchKernelGGL(rigid_tail, dim3(nframes, 2), dim3(256), 0, s, shifts, pixel_spacing, idx_t, w_t, w_y, w_x, nframes,
                     h, w, field, shifts_px, t.S);
  hipLaunchKernelGGL(rigid_weights, dim3((n + 255) / 256, nframes, 2), dim3(256), 0, s, (const float*)shifts_px, nframes,
                     h, w, (const int*)t.S, t.Wy, t.Wx);
  return mc_check_launch();
}

}  // extern "C"
