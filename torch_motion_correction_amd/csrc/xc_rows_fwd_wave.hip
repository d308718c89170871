// K1 of the pruned cross-correlation engine (xc_common.h has the map of the passes), the wave-per-row engine:
// a wavefront per 4096-sample row of a whole frame, fp32 / fp16 / u8 / i16 samples, with or without the fused
// frame statistics (16 kernels: k1_wave_launch instantiates what an entry point can ask for and no more).
// xc_rows_fwd.hip has the entry points and the rules that route a job here and choose its variant.
#include "xc_rows_fwd.h"

// ------------------------------------------------------------------ K1, wave per row
// W = 4096 rows (N = 2048 complex points) with nkx <= 512: one wavefront transforms one
// row on its own (mc_wave_fft.h): no workgroup barrier anywhere in the row loop, 8 KiB of
// LDS per wave, so 12-16 independent row streams per CU keep their HBM loads in flight.
// A workgroup takes WF_ROWS_PER_WG rows in rounds of 8 consecutive rows: wave wv transforms rows 2 wv and
// 2 wv + 1 of a round, and the workgroup writes the round's bins as whole 64-byte pieces of T1[job][kx][y].
// Same arithmetic as xc_rows_fwd up to the summation order of the FFT.

// Scheduling pin: `v` (an index / offset every later address is derived from) becomes
// opaque at the point where `dep` has been computed, so the loads that use it cannot be
// hoisted above that point (the compiler otherwise issues every table read at the top of
// the row and pays for it with ~60 registers each).
__device__ __forceinline__ void wf_pin(int& v, float dep) { asm volatile("" : "+v"(v) : "v"(dep)); }

// Twiddles come from two LDS tables shared by the workgroup's four waves (filled once from
// tw_row, exact table values):
//   twA[s][q]            = W_2048^{q 2^s}        s = 0..3, q < 128     (4 KiB)
//   twB[g][k2 - 1][h]    = W_128^{(2 g + h) k2}  k2 = 1..15            (960 B)
// Lane t reads twA[s][2t..2t+1] and twB[t>>4][k2-1][0..1] as one 16-byte LDS read each
// (the latter a broadcast within 16 lanes).  Pass A's fifteen twiddles W^{q k1} are the four exact
// bases k1 = 1, 2, 4, 8 and eleven products of them (wf_twiddle16, as the 1024- and 4096-point column
// engines do): the table of all fifteen was 15 KiB, and with it a workgroup's 51 KB of LDS allowed three
// workgroups per CU; 40 KB allow four.  The kernel is bound by how many waves are there to issue (49 %
// VALU, 37 % LDS, 62 % of the HBM ceiling; a wave issues at most one VALU instruction per ~6 cycles,
// scripts/ubench/pk_rate.hip), so LDS must never be what keeps a workgroup out of a CU: that is worth more than
// the 44 extra instructions per row.  What the kernel runs is two waves per SIMD -- its 198-235 VGPRs admit two
// workgroups of four waves per CU (WF_MIN_WG), whatever the LDS would allow.
#define WF_TWA (4 * 128)
#define WF_TWB (4 * 15 * 2)
constexpr int WF_ROWS_PER_WG = 32;  // rounds of 8 rows: a wave takes rows 2 wv and 2 wv + 1 of every round (16: the prologue is 22 % of a wave's life; 32: K1 445 -> 430 us)
constexpr int WF_MIN_WG = 2;  // workgroups per CU the register allocation aims at = waves per SIMD (2: up to 256 VGPRs per lane, none of the 16 variants spills; 3: 168, 416 B of scratch)

// N1LO / N1HI: only the 256-sample chunks [N1LO, N1HI) of a row can touch the mask support,
// the others are zero and are not loaded.  CLAMP_ALL = false: the chunks strictly between
// N1LO and N1HI - 1 lie wholly inside the support (host checks) and load unclamped.
// Statistics: box.wl / box.wu are multiples of 256 (host checks), so a chunk is inside
// the box or outside it as a whole.
template <int N1LO, int N1HI, bool CLAMP_ALL, bool HALF = false, int RAW = 0>
__device__ __forceinline__ void wf_load_px(const void* __restrict__ row_any, int t, int xlo, int xhi,
                                           float4 (&px)[16]) {
  if constexpr (RAW == 1) {
    // u8 storage (N2): the lane's four samples are ONE dword, kept raw in px[n1].x and widened where the
    // row is consumed (wf_row), exactly as the fp16 form does
    const unsigned char* row = static_cast<const unsigned char*>(row_any);
#pragma unroll
    for (int n1 = N1LO; n1 < N1HI; ++n1) {
      const int x = 256 * n1 + 4 * t;
      const int xs = (CLAMP_ALL || n1 == N1LO || n1 == N1HI - 1) ? min(max(x, xlo), xhi) : x;
      px[n1].x = __builtin_nontemporal_load(reinterpret_cast<const float*>(row + xs));
    }
    return;
  }
  if constexpr (HALF || RAW == 2) {
    // fp16 storage: the lane's four samples are 8 bytes; they stay RAW in px[n1].x / .y (converting here
    // would make the prefetch wait for its own loads) and are widened where the row is consumed
    const _Float16* row = static_cast<const _Float16*>(row_any);  // (or int16: the same 8 raw bytes)
#pragma unroll
    for (int n1 = N1LO; n1 < N1HI; ++n1) {
      const int x = 256 * n1 + 4 * t;
      typedef float f2 __attribute__((ext_vector_type(2)));
      const int xs = (CLAMP_ALL || n1 == N1LO || n1 == N1HI - 1) ? min(max(x, xlo), xhi) : x;
      const f2 q = __builtin_nontemporal_load(reinterpret_cast<const f2*>(row + xs));
      px[n1].x = q.x;
      px[n1].y = q.y;
    }
    return;
  }
  const float* row = static_cast<const float*>(row_any);
  // Branch-free: a lane whose quad lies outside [xlo, xhi + 4) -- the support box, or with
  // CLAMP_ALL and a chord table this row's own chord of the mask disk -- reads the nearest quad
  // inside it instead (a line its neighbours fetch anyway: no extra HBM traffic); the value
  // is later multiplied by the mask's exact zero.
#pragma unroll
  for (int n1 = N1LO; n1 < N1HI; ++n1) {
    const int x = 256 * n1 + 4 * t;
    // read-once stream: non-temporal, so that it does not push the mask rows out of L2
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int xs = (CLAMP_ALL || n1 == N1LO || n1 == N1HI - 1) ? min(max(x, xlo), xhi) : x;
    const f4 q = __builtin_nontemporal_load(reinterpret_cast<const f4*>(row + xs));
    px[n1] = make_float4(q.x, q.y, q.z, q.w);
  }
}

template <int N1LO, int N1HI>
__device__ __forceinline__ void wf_load_mask(const float* __restrict__ mrow, int t, float4 (&mk)[16]) {
  // mask rows (L2-resident) are read as they are: exact zeros outside the support
#pragma unroll
  for (int n1 = N1LO; n1 < N1HI; ++n1) mk[n1] = *reinterpret_cast<const float4*>(mrow + 256 * n1 + 4 * t);
}

// raw bits of two fp16 samples -> two floats
__device__ __forceinline__ wf2 wf_unpack_h2(float bits) {
  const unsigned v = __float_as_uint(bits);
  return wf2{(float)__builtin_bit_cast(_Float16, (unsigned short)(v & 0xffffu)),
             (float)__builtin_bit_cast(_Float16, (unsigned short)(v >> 16))};
}

// raw bits of four u8 samples (one dword) / two i16 samples -> floats
__device__ __forceinline__ void wf_unpack_u8x4(float bits, wf2& a01, wf2& a23) {
  const unsigned v = __float_as_uint(bits);
  a01 = wf2{(float)(v & 0xffu), (float)((v >> 8) & 0xffu)};
  a23 = wf2{(float)((v >> 16) & 0xffu), (float)(v >> 24)};
}
__device__ __forceinline__ wf2 wf_unpack_i16x2(float bits) {
  const unsigned v = __float_as_uint(bits);
  return wf2{(float)(short)(v & 0xffffu), (float)((int)v >> 16)};
}

// One row.  px holds this row's samples on entry and the next row's on exit (loaded right after the current
// ones were consumed, so the HBM latency of row i+1 hides behind the transform of row i; loading them here, or
// prefetching the mask row as well, measured slower).  next_row is null after the last row (wave-uniform).
template <int KEEP, bool STATS, int N1LO, int N1HI, bool CLAMP_ALL, bool HALF = false, int RAW = 0>
__device__ __forceinline__ void wf_row(float4 (&px)[16], float4 (&mk)[16], const float* __restrict__ mrow,
                                       const void* __restrict__ next_row, int t, wf2* slab,
                                       const cfloat* twA, const cfloat* twB, const cfloat* twK,
                                       const XcGeom& g, int box_lo, int box_hi, float mean, float rstd,
                                       float& st_s, float& st_q, wf2 (&X)[4][KEEP], int xlo, int xhi,
                                       int nxlo, int nxhi, const float* __restrict__ grow = nullptr) {
  wf2 A0[16], A1[16];
  if constexpr (RAW != 0) {
    // N2: A = (raw * gain - sub_f) * rstd * mask, `mean` = sub_f = frame mean + box mean (mc_raw_movie_stats).
    // Gain and mask values are fetched and consumed in two half-row groups: all 32 float4 of a row at
    // once would be 128 registers next to the 64 of A0 / A1.
    auto half_row = [&](auto lo_tag) {
      constexpr int LO = decltype(lo_tag)::value, HI = LO + 8;
      float4 gq[8], mq[8];
#pragma unroll
      for (int n1 = LO; n1 < HI; ++n1) {
        if (n1 >= N1LO && n1 < N1HI) {
          const int x = 256 * n1 + 4 * t;
          const int xs = (CLAMP_ALL || n1 == N1LO || n1 == N1HI - 1) ? min(max(x, xlo), xhi) : x;
          gq[n1 - LO] = *reinterpret_cast<const float4*>(grow + xs);  // the sample's own (clamped) column
          mq[n1 - LO] = *reinterpret_cast<const float4*>(mrow + x);
        }
      }
#pragma unroll
      for (int n1 = LO; n1 < HI; ++n1) {
        if (n1 >= N1LO && n1 < N1HI) {
          wf2 r01, r23;
          if constexpr (RAW == 1) wf_unpack_u8x4(px[n1].x, r01, r23);
          else { r01 = wf_unpack_i16x2(px[n1].x); r23 = wf_unpack_i16x2(px[n1].y); }
          const float4 gv = gq[n1 - LO], mv = mq[n1 - LO];
          const wf2 a01 = __builtin_elementwise_fma(r01, wf2{gv.x, gv.y}, wf2{-mean, -mean});
          const wf2 a23 = __builtin_elementwise_fma(r23, wf2{gv.z, gv.w}, wf2{-mean, -mean});
          A0[n1] = (a01 * rstd) * wf2{mv.x, mv.y};
          A1[n1] = (a23 * rstd) * wf2{mv.z, mv.w};
        } else {
          A0[n1] = wf2{0.f, 0.f};
          A1[n1] = wf2{0.f, 0.f};
        }
      }
    };
    half_row(std::integral_constant<int, 0>{});
    {
      int tp = t;
      wf_pin(tp, A1[7].y);  // the second group's loads start once the first group has been consumed
      t = tp;
    }
    half_row(std::integral_constant<int, 8>{});
  }
  if (RAW == 0) wf_load_mask<N1LO, N1HI>(mrow, t, mk);
  if constexpr (STATS && RAW == 0) {
    // The statistics of a row of the box (wave-uniform) are taken from px under the mask loads' latency, in a
    // side block of their own: the conditioning below is then the same straight-line code as without STATS.
    // As one block per kind of row, each with its own copy of the conditioning, the compiler kept both copies'
    // 64 results apart and the full-width variants went to scratch.  The centred samples are formed twice on
    // these rows, by the same subtraction, so every sum keeps its bits.
    if (box_hi > box_lo) {
      wf2 acc_s = {0.f, 0.f}, acc_q = {0.f, 0.f};
#pragma unroll
      for (int n1 = N1LO; n1 < N1HI; ++n1) {
        const wf2 a01 = (HALF ? wf_unpack_h2(px[n1].x) : wf2{px[n1].x, px[n1].y}) - mean;
        const wf2 a23 = (HALF ? wf_unpack_h2(px[n1].y) : wf2{px[n1].z, px[n1].w}) - mean;
        // chunk weight 1 inside the box, 0 outside (scalar): no branch per chunk
        const float cw = (n1 >= box_lo && n1 < box_hi) ? 1.f : 0.f;
        const wf2 sa = a01 + a23;
        const wf2 sq = __builtin_elementwise_fma(a01, a01, a23 * a23);
        acc_s = __builtin_elementwise_fma(sa, wf2{cw, cw}, acc_s);
        acc_q = __builtin_elementwise_fma(sq, wf2{cw, cw}, acc_q);
      }
      st_s += acc_s.x + acc_s.y;
      st_q += acc_q.x + acc_q.y;
    }
  }
  if constexpr (RAW == 0) {
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {
      if (n1 >= N1LO && n1 < N1HI) {
        const wf2 a01 = (HALF ? wf_unpack_h2(px[n1].x) : wf2{px[n1].x, px[n1].y}) - mean;
        const wf2 a23 = (HALF ? wf_unpack_h2(px[n1].y) : wf2{px[n1].z, px[n1].w}) - mean;
        A0[n1] = (a01 * rstd) * wf2{mk[n1].x, mk[n1].y};
        A1[n1] = (a23 * rstd) * wf2{mk[n1].z, mk[n1].w};
      } else {
        A0[n1] = wf2{0.f, 0.f};
        A1[n1] = wf2{0.f, 0.f};
      }
    }
  }
  int tl = t;  // lane index as the tables see it (re-pinned before each table)
  wf_pin(tl, A0[N1HI - 1].x);
  const WfLane L = wf_lane(tl);  // slab addresses: derived here, not carried across rows
  if (next_row) {  // issued once this row's samples have been consumed, not earlier
    int tp = t;
    wf_pin(tp, A1[N1HI - 1].y);
    wf_load_px<N1LO, N1HI, CLAMP_ALL, HALF, RAW>(next_row, tp, nxlo, nxhi, px);
  }
  wf_dft16(A0);
  wf_pin(tl, A0[15].y);  // table reads fly under the second butterfly
  {
    const float4* twa = reinterpret_cast<const float4*>(twA) + tl;  // [s][64 lanes] of 16 B: q = 2 t, 2 t + 1
    float4 w[4];
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) w[sb] = twa[sb * 64];
    wf_dft16(A1);
    wf_twiddle16(A0, wf2{w[0].x, w[0].y}, wf2{w[1].x, w[1].y}, wf2{w[2].x, w[2].y}, wf2{w[3].x, w[3].y});
    wf_twiddle16(A1, wf2{w[0].z, w[0].w}, wf2{w[1].z, w[1].w}, wf2{w[2].z, w[2].w}, wf2{w[3].z, w[3].w});
  }

  wf2 B0[16], B1[16];
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) slab[L.x1w_base + (k1 ^ L.x1w_mask)] = A0[k1];
  wf_sync();
#pragma unroll
  for (int n2 = 0; n2 < 16; ++n2) B0[n2] = slab[L.x1r[n2 & 3] + 64 * n2];
  wf_sync();
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) slab[L.x1w_base + (k1 ^ L.x1w_mask)] = A1[k1];
  wf_sync();
  wf_dft16(B0);
#pragma unroll
  for (int n2 = 0; n2 < 16; ++n2) B1[n2] = slab[L.x1r[n2 & 3] + 64 * n2];
  wf_sync();
  wf_pin(tl, B0[15].y);
  {
    const float4* twb = reinterpret_cast<const float4*>(twB) + (tl >> 4) * 15;
    float4 w[15];
#pragma unroll
    for (int k2 = 1; k2 < 16; ++k2) w[k2 - 1] = twb[k2 - 1];
    wf_dft16(B1);
#pragma unroll
    for (int k2 = 1; k2 < 16; ++k2) {
      B0[k2] = wf_cmul(B0[k2], wf2{w[k2 - 1].x, w[k2 - 1].y});
      B1[k2] = wf_cmul(B1[k2], wf2{w[k2 - 1].z, w[k2 - 1].w});
    }
  }
#pragma unroll
  for (int k2 = 0; k2 < 16; ++k2) slab[L.x2w + 16 * k2] = B0[k2];
  wf_sync();
  wf2 Ce[4][4], Co[4][4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int n3h = 0; n3h < 4; ++n3h) Ce[s][n3h] = slab[L.x2r[s] + 256 * n3h];
  wf_sync();
#pragma unroll
  for (int k2 = 0; k2 < 16; ++k2) slab[L.x2w + 16 * k2] = B1[k2];
  wf_sync();
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int n3h = 0; n3h < 4; ++n3h) Co[s][n3h] = slab[L.x2r[s] + 256 * n3h];
  wf_sync();
  wf_pin(tl, Ce[0][0].x);
  wf2 z[4][8], wk[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    wk[s] = wf_from(twK[64 * s + tl]);
    wf_dft8_pruned<KEEP>(Ce[s], Co[s], z[s]);
  }
  wf_unpack_lane<KEEP>(z, wk, L.self != 0, X);
}

// RAW (N2): 1 = u8, 2 = i16 samples conditioned on the fly: `gain` is the (h, row_stride) gain reference
// (same row pitch as the frames: whole-frame jobs), `job_sub[job]` the per-frame offset, mean_rstd[1]
// the scale (mc_raw_movie_stats); no statistics are gathered.
template <int KEEP, bool STATS, int N1LO, int N1HI, bool CLAMP_ALL, bool HALF = false, int RAW = 0>
__global__ __launch_bounds__(256, WF_MIN_WG) void xc_rows_fwd_wave(
    const void* __restrict__ src, const int64_t* __restrict__ job_off, int64_t row_stride,
    const float* __restrict__ mask, const float* __restrict__ mean_rstd, cfloat* __restrict__ T1,
    const cfloat* __restrict__ tw_row, XcGeom g, XcBox box, double* __restrict__ stats_acc,
    const int2* __restrict__ chord, const float* __restrict__ gain, const float* __restrict__ job_sub) {
  __shared__ __attribute__((aligned(16))) cfloat slabs[4][WF_SLAB];
  __shared__ __attribute__((aligned(16))) cfloat tab[WF_TWA + WF_TWB + 256];
  const cfloat* twA = tab;
  const cfloat* twB = tab + WF_TWA;
  const cfloat* twK = tab + WF_TWA + WF_TWB;  // [slot][lane] = w^kbin
  const int t = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  wf2* slab = reinterpret_cast<wf2*>(slabs[wv]);
  // Workgroup -> (job, row group): workgroups are dealt round-robin over the 8 XCDs (speed
  // only, MI355X guide), so every job of one row group is sent to the same XCD: its L2 then
  // fetches the group's mask rows once for all jobs instead of once per XCD.
  const int njobs = gridDim.y;
  const int b = blockIdx.x + gridDim.x * blockIdx.y;  // gridDim.x = 8 * ceil(groups / 8)... see host
  const int grp = 8 * (b / (8 * njobs)) + (b & 7);
  const int job = (b >> 3) % njobs;
  if (grp * WF_ROWS_PER_WG >= g.ny) return;  // padding of the last eight groups (uniform)
  {  // tables from tw_row[k] = exp(-2 pi i k / 4096): W_2048^m = tw_row[2 m], W_128^m =
     // tw_row[32 m]; all loads issued before the first LDS write
    constexpr int NTAB = WF_TWA + WF_TWB + 256, PER = (NTAB + 255) / 256;
    cfloat tv[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      int i = threadIdx.x + 256 * j;
      i = i < NTAB ? i : NTAB - 1;
      int src_k;
      if (i < WF_TWA) {
        src_k = (2 * (i & 127)) << (i >> 7);  // W_2048^{q 2^s} = tw_row[2 q 2^s]
      } else if (i < WF_TWA + WF_TWB) {
        const int e = i - WF_TWA, h = e & 1, k2 = ((e >> 1) % 15) + 1, gq = e / 30;
        src_k = 32 * (2 * gq + h) * k2;
      } else {
        const int e = i - WF_TWA - WF_TWB, sl = e >> 6, l = e & 63;
        src_k = sl == 0 ? l : (sl == 1 ? (l == 0 ? 128 : 256 - l) : (sl == 2 ? 64 + l : 192 - l));
      }
      tv[j] = tw_row[src_k];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = threadIdx.x + 256 * j;
      if (i < NTAB) tab[i] = tv[j];
    }
  }
  const float mean = RAW ? job_sub[job] : (mean_rstd ? mean_rstd[0] : 0.f);
  const float rstd = mean_rstd ? mean_rstd[1] : 1.f;
  // frames in their storage type: fp32, or (HALF) fp16 / (RAW) u8, i16 read as they are; job_off / row_stride in samples
  constexpr int SB = RAW == 1 ? 1 : (HALF || RAW == 2) ? 2 : 4;
  const char* base = static_cast<const char*>(src) + job_off[job] * SB;
  auto row_at = [&](int y) -> const void* { return base + (int64_t)y * row_stride * SB; };
  float st_s = 0.f, st_q = 0.f;
  cfloat* out = T1 + (int64_t)job * g.nkx * g.ny;
  // A workgroup takes WF_ROWS_PER_WG rows in rounds of 8 consecutive rows; in a round wave wv
  // transforms rows 2 wv and 2 wv + 1, parks their bins in its own slab as [kx][2 rows] and
  // the workgroup then writes T1[job][kx][8 rows] as whole 64-byte pieces (every byte of T1
  // written once; scattered 16-byte stores cost 2.8x the bytes at the memory side).
  const int r16 = grp * WF_ROWS_PER_WG;
  auto row_of = [&](int i) { return r16 + (i >> 1) * 8 + 2 * wv + (i & 1); };  // i = 0..3
  const int rounds_left = (g.ny - r16) >> 3;  // ny % 8 == 0
  const int nrows = 2 * (rounds_left < WF_ROWS_PER_WG / 8 ? rounds_left : WF_ROWS_PER_WG / 8);
  float4 px[16], mk[16];
  // clamp bounds of a row's sample loads: the support box, or (CLAMP_ALL with a table) the row's
  // own chord of the mask disk -- the corners of the box, 21 % of it, are then never fetched
  const int bxlo = g.x0 & ~3, bxhi = ((g.x1 + 3) & ~3) - 4;
  auto bounds = [&](int y) { return (CLAMP_ALL && chord) ? chord[y] : make_int2(bxlo, bxhi); };
  if (nrows > 0) {
    const int2 c0 = bounds(g.y0 + row_of(0));
    wf_load_px<N1LO, N1HI, CLAMP_ALL, HALF, RAW>(row_at(g.y0 + row_of(0)), t, c0.x, c0.y, px);
  }
  __syncthreads();
  wf2 Xe[4][KEEP];  // bins of the even row of the current pair
#pragma unroll 1
  for (int rr = 0; rr < nrows; ++rr) {
    const int y = g.y0 + row_of(rr);
    const float* mrow = mask + (int64_t)y * g.W;
    const int yn = g.y0 + row_of(rr + 1);
    const void* next_row = rr + 1 < nrows ? row_at(yn) : nullptr;
    const bool in_box_row = STATS && y >= box.hl && y < box.hu;
    wf2 X[4][KEEP];
    const int2 cb = bounds(y), cn = bounds(rr + 1 < nrows ? yn : y);
    wf_row<KEEP, STATS, N1LO, N1HI, CLAMP_ALL, HALF, RAW>(
        px, mk, mrow, next_row, t, slab, twA, twB, twK, g, box.wl >> 8,
        in_box_row ? (box.wu >> 8) : 0, mean, rstd, st_s, st_q, X, cb.x, cb.y, cn.x, cn.y,
        RAW ? gain + (int64_t)y * row_stride : nullptr);
    if (rr & 1) {
      int ts = t;
      wf_pin(ts, X[0][0].x);  // addresses: computed here, not carried across rows
      const WfLane L = wf_lane(ts);
      float4* park = reinterpret_cast<float4*>(slab);  // [kx] = {even row, odd row}
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int k3 = 0; k3 < KEEP; ++k3) {
          const int k = L.kbin[s] + 256 * k3;
          if (k < g.nkx) park[k] = make_float4(Xe[s][k3].x, Xe[s][k3].y, X[s][k3].x, X[s][k3].y);
        }
      __syncthreads();
      int tj = threadIdx.x;
      wf_pin(tj, X[0][0].y);
      const float4* parked = reinterpret_cast<const float4*>(&slabs[0][0]);
      const int r8 = r16 + (rr >> 1) * 8;
      // 4 lanes = the 64 bytes of one kx; nkx <= 256 KEEP, so at most 4 KEEP pieces per thread: all the
      // LDS reads first, then the stores (one LDS latency per round instead of one per piece).  The reads are
      // unconditional (j < 2048: always inside slabs[][]; only the store is guarded): read under `j < 4 nkx`
      // the 16 values were undefined on the other path and the compiler kept them alive round the whole row
      // loop -- 16 VGPRs in every variant, and the scratch of the statistics variants at the 256 limit
      typedef float f4 __attribute__((ext_vector_type(4)));
#pragma unroll
      for (int half = 0; half < KEEP; ++half) {  // four pieces (16 registers) at a time
        float4 pv[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int j = tj + 256 * (4 * half + it);
          pv[it] = parked[(j & 3) * (WF_SLAB / 2) + (j >> 2)];
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int j = tj + 256 * (4 * half + it);
          if (j < 4 * g.nkx) {
            const int kx = j >> 2, w = j & 3;
            // T1 is written once here and read once by K2, 0.4 GB later: non-temporal (K1 0.465 -> 0.455 ms)
            const f4 v = {pv[it].x, pv[it].y, pv[it].z, pv[it].w};
            __builtin_nontemporal_store(v, reinterpret_cast<f4*>(out + (int64_t)kx * g.ny + r8 + 2 * w));
          }
        }
      }
      __syncthreads();
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int k3 = 0; k3 < KEEP; ++k3) Xe[s][k3] = X[s][k3];
    }
  }
  if constexpr (STATS) {
    double ds = st_s, dq = st_q;
    for (int o = 32; o > 0; o >>= 1) {
      ds += __shfl_down(ds, o);
      dq += __shfl_down(dq, o);
    }
    __shared__ double rs[4], rq[4];
    if (t == 0) {
      rs[wv] = ds;
      rq[wv] = dq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      ds = (rs[0] + rs[1]) + (rs[2] + rs[3]);
      dq = (rq[0] + rq[1]) + (rq[2] + rq[3]);
      if (ds != 0.0 || dq != 0.0) {
        const int slot = (blockIdx.x + 7 * blockIdx.y) & (XC_STAT_SLOTS - 1);
        atomicAdd(&stats_acc[2 * slot], ds);
        atomicAdd(&stats_acc[2 * slot + 1], dq);
      }
    }
  }
}

// ------------------------------------------------------------------ host side
static dim3 wave_rows_grid(const XcGeom& g, int njobs) {  // linear id = x + gridDim.x * y, decoded in the kernel
  const int ngroups = (g.ny + WF_ROWS_PER_WG - 1) / WF_ROWS_PER_WG;
  return dim3((ngroups + 7) / 8 * 8, njobs);
}

int k1_wave_launch(K1WaveVariant v, int raw, const void* src, const int64_t* job_off, int64_t row_stride,
                   const float* mask, const float* mean_rstd, void* T1, const void* tw_row, int njobs, const XcGeom& g,
                   const XcBox& b, double* stats_acc, const int* row_chord, const float* gain, const float* job_sub,
                   void* stream) {
  // fp16 samples and chord-clamped inner chunks come with statistics only (mc_xc_rows_forward takes neither fp16
  // samples nor a chord table): without statistics there is no such kernel
  if (!raw && !stats_acc && (v.loads == K1_LOADS_HALF || v.loads == K1_LOADS_INNER_CHORD)) return MC_ERR_UNSUPPORTED;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, wave_rows_grid(g, njobs), dim3(256), 0, (hipStream_t)stream, src, job_off, row_stride,
                       mask, mean_rstd, (cfloat*)T1, (const cfloat*)tw_row, g, b, stats_acc, (const int2*)row_chord,
                       gain, job_sub);
  };
  mc_pick(v.keep1, [&](auto keep1) {
    constexpr int KEEP = decltype(keep1)::value ? 1 : 2;
    if (raw) {  // u8 / i16: the general variant, no statistics
      mc_pick(raw == 1, [&](auto is_u8) {
        launch(xc_rows_fwd_wave<KEEP, false, 0, 16, true, false, decltype(is_u8)::value ? 1 : 2>);
      });
      return;
    }
    mc_pick(stats_acc != nullptr, [&](auto stats) {
      constexpr bool ST = decltype(stats)::value;
      switch (v.loads) {
        case K1_LOADS_HALF:
          if constexpr (ST) launch(xc_rows_fwd_wave<KEEP, ST, 0, 16, true, true>);
          break;
        case K1_LOADS_INNER_CHORD:
          if constexpr (ST) launch(xc_rows_fwd_wave<KEEP, ST, 1, 15, true>);
          break;
        case K1_LOADS_INNER: launch(xc_rows_fwd_wave<KEEP, ST, 1, 15, false>); break;
        default: launch(xc_rows_fwd_wave<KEEP, ST, 0, 16, true>); break;
      }
    });
  });
  return mc_check_launch();
}
