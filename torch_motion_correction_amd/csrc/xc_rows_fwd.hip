// K1 of the pruned cross-correlation engine (xc_common.h has the map of the passes): forward row transforms,
//   gather + (x - mean) * rstd * mask^e -> real FFT(W) -> first nkx bins -> T1[job][kx][ysupport]
// by three engines -- a workgroup per row group (any power-of-two width), a wavefront per 4096-sample row
// and a wavefront per 1024-sample patch row -- the kernels of the fused frame statistics, and the hot-pixel
// correction of a raw movie's T1.
#include "xc_common.h"

// ------------------------------------------------------------------ K1: rows forward
// Two LDS lines (ping-pong: one barrier per pass), twiddles in registers for the whole
// row loop, and the next row's samples + mask values already in flight (registers)
// while the current row is transformed.


// Sub-groups: fft_threads(N) threads cooperate on one row, MC_WG / that many rows are in
// flight per workgroup (N = 2048: the whole workgroup on one row; N = 512: one wavefront
// per row, four rows at a time).  Each sub-group owns a pair of LDS lines (ping-pong: one
// barrier per pass); twiddles live in registers for the whole row loop.
// RAW (N2): 1 = u8, 2 = i16 samples conditioned on the fly as raw * gain - job_sub[job] (whole-frame jobs:
// `gain` has the frames' row pitch); no statistics then.
template <int LOGN, bool STATS, int RAW = 0>
__global__ __launch_bounds__(MC_WG) void xc_rows_fwd(
    const void* __restrict__ src_any, const int64_t* __restrict__ job_off, int64_t row_stride,
    const int* __restrict__ job_expo, const float* __restrict__ mask,
    const float* __restrict__ mean_rstd, cfloat* __restrict__ T1,
    const cfloat* __restrict__ tw_row, XcGeom g, XcBox box, double* __restrict__ stats_acc,
    const float* __restrict__ gain, const float* __restrict__ job_sub) {
  constexpr int N = 1 << LOGN;  // complex length = W/2
  constexpr int NT = fft_threads(N), SG = MC_WG / NT;
  constexpr int R0 = FftPlan<N>::radix(0), NB0 = N / R0, IT0 = (NB0 + NT - 1) / NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lt = tid & (NT - 1), sg = tid / NT;
  cfloat* l0 = reinterpret_cast<cfloat*>(smem) + sg * 2 * lds_len(N);
  cfloat* l1 = l0 + lds_len(N);
  cfloat* stg = reinterpret_cast<cfloat*>(smem) + SG * 2 * lds_len(N);
  // job is the fastest grid dimension: the workgroups that share a row group's mask rows
  // (one per job) are dispatched together and find them in L2
  const int job = blockIdx.x;
  const int grp = blockIdx.y;
  const int RG = g.RG;
  const float mean = RAW ? job_sub[job] : (mean_rstd ? mean_rstd[0] : 0.f);
  const float rstd = mean_rstd ? mean_rstd[1] : 1.f;
  const int expo = job_expo ? job_expo[job] : (mask ? 1 : 0);
  constexpr int SB = RAW == 1 ? 1 : RAW == 2 ? 2 : 4;
  const char* base = static_cast<const char*>(src_any) + job_off[job] * SB;
  FftTwiddles<N> T;
  T.template init<-1>(lt, tw_row, 2);

  int s = 0;
  float st_s = 0.f, st_q = 0.f;  // sum and sum of squares of (x - mean_rstd[0]) inside the box
  for (int r = sg; r < RG; r += SG) {  // RG % SG == 0: every sub-group runs the same trip count
    const int y = g.y0 + grp * RG + r;
    const char* rowb = base + (int64_t)y * row_stride * SB;
    const float* grow = RAW ? gain + (int64_t)y * row_stride : nullptr;
    auto row_at = [&](int xx) -> float {
      if constexpr (RAW == 1) return (float)reinterpret_cast<const unsigned char*>(rowb)[xx] * grow[xx];
      else if constexpr (RAW == 2) return (float)reinterpret_cast<const short*>(rowb)[xx] * grow[xx];
      else return reinterpret_cast<const float*>(rowb)[xx];
    };
    const float* mrow = mask + (int64_t)y * g.W;
    cfloat px[IT0][R0], mk[IT0][R0];
#pragma unroll
    for (int it = 0; it < IT0; ++it) {
      const int j = lt + it * NT;
#pragma unroll
      for (int q = 0; q < R0; ++q) {
        const int x = 2 * (j + q * NB0);
        const bool on = (NB0 % NT == 0 || j < NB0) && x >= g.x0 && x < g.x1;
        px[it][q] = on ? cmake(row_at(x), row_at(x + 1)) : cmake(mean, mean);
        mk[it][q] = (on && expo > 0) ? cmake(mrow[x], mrow[x + 1]) : cmake(on ? 1.f : 0.f, on ? 1.f : 0.f);
      }
    }
    if constexpr (STATS) {
      if (y >= box.hl && y < box.hu) {
#pragma unroll
        for (int it = 0; it < IT0; ++it)
#pragma unroll
          for (int q = 0; q < R0; ++q) {
            const int x = 2 * (lt + it * NT + q * NB0);
            if ((NB0 % NT == 0 || lt + it * NT < NB0) && x >= box.wl && x < box.wu) {
              // box.wl/wu are even (host guarantees), so x+1 is inside too
              const float a = px[it][q].x - mean, b = px[it][q].y - mean;
              st_s += a + b;
              st_q += a * a + b * b;
            }
          }
      }
    }
    auto load = [&](int, int it, int q) {
      cfloat v = cmake((px[it][q].x - mean) * rstd, (px[it][q].y - mean) * rstd);
      const cfloat mm = mk[it][q];
      v.x *= mm.x;
      v.y *= mm.y;
      for (int e = 1; e < expo; ++e) {
        v.x *= mm.x;
        v.y *= mm.y;
      }
      return v;
    };
    auto nostore = [](int, cfloat) {};
    const int res = wg_fft_pp<N, -1, false>(l0, l1, s, lt, T, load, nostore);
    const cfloat* Z = res ? l1 : l0;
    // real-FFT unpack: X[k] = (Z[k] + conj(Z[N-k]))/2 - i/2 * w^k * (Z[k] - conj(Z[N-k]))
    for (int k = lt; k < g.nkx; k += NT) {
      const cfloat zk = Z[lpad(k & (N - 1))];
      const cfloat zm = cconj(Z[lpad((N - k) & (N - 1))]);
      const cfloat sm = cadd(zk, zm), d = csub(zk, zm);
      const cfloat w = (k < N) ? tw_row[k] : cmake(-1.f, 0.f);
      const cfloat wd = cmul(w, d);  // -i*wd = (wd.y, -wd.x)
      stg[k * (RG + 1) + r] = cmake(0.5f * (sm.x + wd.y), 0.5f * (sm.y - wd.x));
    }
    s = res ^ 1;  // next row must not start in the line that is still being unpacked
  }
  __syncthreads();
  cfloat* out = T1 + (int64_t)job * g.nkx * g.ny + (int64_t)grp * RG;
  for (int i = tid; i < g.nkx * RG; i += MC_WG) {
    const int kx = i / RG, r = i - kx * RG;
    out[(int64_t)kx * g.ny + r] = stg[kx * (RG + 1) + r];
  }
  if constexpr (STATS) {
    double ds = st_s, dq = st_q;
    for (int off = 32; off > 0; off >>= 1) {
      ds += __shfl_down(ds, off);
      dq += __shfl_down(dq, off);
    }
    __shared__ double rs[MC_WG / 64], rq[MC_WG / 64];
    if ((tid & 63) == 0) {
      rs[tid >> 6] = ds;
      rq[tid >> 6] = dq;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < MC_WG / 64; ++w) {
        ds += rs[w];
        dq += rq[w];
      }
      if (ds != 0.0 || dq != 0.0) {
        atomicAdd(&stats_acc[0], ds);
        atomicAdd(&stats_acc[1], dq);
      }
    }
  }
}

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

#define XC_STAT_SLOTS 64  // stats_acc = XC_STAT_SLOTS x {sum, sumsq} doubles

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
// scripts/ubench/pk_rate.hip), so the fourth wave per SIMD is worth more than the 44 extra instructions
// per row.
#define WF_TWA (4 * 128)
#define WF_TWB (4 * 15 * 2)
constexpr int WF_ROWS_PER_WG = 32;  // rounds of 8 rows: a wave takes rows 2 wv and 2 wv + 1 of every round (16: the prologue is 22 % of a wave's life; 32: K1 445 -> 430 us)
constexpr int WF_MIN_WG = 2;  // workgroups per CU the register allocation aims at (2: 256 VGPRs per lane, 3: 168)

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
  auto condition = [&](auto in_box) {
    constexpr bool INBOX = decltype(in_box)::value;
    wf2 acc_s = {0.f, 0.f}, acc_q = {0.f, 0.f};
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {
      if (n1 >= N1LO && n1 < N1HI) {
        const wf2 a01 = (HALF ? wf_unpack_h2(px[n1].x) : wf2{px[n1].x, px[n1].y}) - mean;
        const wf2 a23 = (HALF ? wf_unpack_h2(px[n1].y) : wf2{px[n1].z, px[n1].w}) - mean;
        if (INBOX) {  // chunk weight 1 inside the box, 0 outside (scalar): no branch per chunk
          const float cw = (n1 >= box_lo && n1 < box_hi) ? 1.f : 0.f;
          const wf2 sa = a01 + a23;
          const wf2 sq = __builtin_elementwise_fma(a01, a01, a23 * a23);
          acc_s = __builtin_elementwise_fma(sa, wf2{cw, cw}, acc_s);
          acc_q = __builtin_elementwise_fma(sq, wf2{cw, cw}, acc_q);
        }
        A0[n1] = (a01 * rstd) * wf2{mk[n1].x, mk[n1].y};
        A1[n1] = (a23 * rstd) * wf2{mk[n1].z, mk[n1].w};
      } else {
        A0[n1] = wf2{0.f, 0.f};
        A1[n1] = wf2{0.f, 0.f};
      }
    }
    if (INBOX) {
      st_s += acc_s.x + acc_s.y;
      st_q += acc_q.x + acc_q.y;
    }
  };
  if constexpr (RAW == 0) {
    if (STATS && box_hi > box_lo) condition(std::true_type{});  // wave-uniform: a row of the box
    else condition(std::false_type{});
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
    const int2* __restrict__ chord, int lines16, const float* __restrict__ gain,
    const float* __restrict__ job_sub) {
  extern __shared__ __attribute__((aligned(16))) float4 park0[];  // lines16: [4 waves][nkx]
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
      // lines16: the first round's bins wait in their own LDS area (park0, dynamic) until the second
      // round is done, and T1[job][kx][16 rows] goes out as whole 128-byte lines (two 64-byte halves
      // written 10 us apart merged in L2 only most of the time: 0.55 GB written for a 0.40 GB T1)
      const bool hold = lines16 && nrows == 4 && rr == 1;
      float4* park = hold ? park0 + wv * g.nkx : reinterpret_cast<float4*>(slab);  // [kx] = {even row, odd row}
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int k3 = 0; k3 < KEEP; ++k3) {
          const int k = L.kbin[s] + 256 * k3;
          if (k < g.nkx) park[k] = make_float4(Xe[s][k3].x, Xe[s][k3].y, X[s][k3].x, X[s][k3].y);
        }
      if (!hold) {  // workgroup-uniform
        __syncthreads();
        int tj = threadIdx.x;
        wf_pin(tj, X[0][0].y);
        const float4* parked = reinterpret_cast<const float4*>(&slabs[0][0]);
        if (lines16 && nrows == 4) {
          for (int j = tj; j < 8 * g.nkx; j += 256) {  // 8 lanes = the 128 bytes of one kx
            const int kx = j >> 3, pc = j & 7, w = pc & 3;
            const float4 v = (pc >> 2) ? parked[w * (WF_SLAB / 2) + kx] : park0[w * g.nkx + kx];
            *reinterpret_cast<float4*>(out + (int64_t)kx * g.ny + r16 + 2 * pc) = v;
          }
        } else {
          const int r8 = r16 + (rr >> 1) * 8;
          // 4 lanes = the 64 bytes of one kx; nkx <= 256 KEEP, so at most 4 KEEP pieces per thread: all the
          // LDS reads first, then the stores (one LDS latency per round instead of one per piece)
          typedef float f4 __attribute__((ext_vector_type(4)));
#pragma unroll
          for (int half = 0; half < KEEP; ++half) {  // four pieces (16 registers) at a time
            float4 pv[4];
#pragma unroll
            for (int it = 0; it < 4; ++it) {
              const int j = tj + 256 * (4 * half + it);
              if (j < 4 * g.nkx) pv[it] = parked[(j & 3) * (WF_SLAB / 2) + (j >> 2)];
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
        }
        __syncthreads();
      }
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

// ------------------------------------------------------------------ K1, wave per 1024-sample row
// Patch rows (W = 1024, N = 512 complex points, nkx <= 128): the 8 x 8 x 8 variant of the
// wave engine (mc_wave_fft.h, second half) -- eight complex values per lane, one radix-8
// butterfly per lane and pass, a 4 KiB slab per wave.  DUAL: the same samples are transformed
// twice, with mask^ea and mask^eb (the U and V spectra of the mean-except-current reference,
// estimate_motion_xc.py:315-346), so the patch rows are read once instead of twice.
// Exponents must be >= 1 (the mask's exact zeros outside its support do the windowing).
#define WF5_TWA (7 * 64)
#define WF5_TWB (8 * 7)
#define WF5_TWK 128
constexpr int WF5_MIN_WAVES = 5;  // waves per SIMD the register allocation aims at (DUAL fp32 sits at 97 VGPRs without it: 4)
#define WF5_ROWS_PER_WG 32  // rounds of 8 rows: wave wv takes rows 2 wv and 2 wv + 1 of a round

__device__ __forceinline__ wf2 wf5_ld2(const float* p) {  // 4-byte aligned 8-byte load
  wf2 v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
// two adjacent samples of fp16 storage (a 2-byte aligned 4-byte load), widened to fp32: the
// reference has no fp16 path at all (rfftn rejects Half on the CPU); the result is what
// it computes on the fp32 up-cast of the same stack
typedef _Float16 wf_h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ wf2 wf5_ld2h(const _Float16* p) {
  wf_h2 v;
  __builtin_memcpy(&v, p, 4);
  return wf2{(float)v.x, (float)v.y};
}

__device__ __forceinline__ void wf5_fft(wf2 (&A)[8], int t, wf2* slab, const wf2* twA, const wf2* twB,
                                        const wf2* twK, wf2 (&X)[2]) {
  const int lo = t & 7, hi = t >> 3;
  wf_dft8(A);
#pragma unroll
  for (int k1 = 1; k1 < 8; ++k1) A[k1] = wf_cmul(A[k1], twA[(k1 - 1) * 64 + t]);
#pragma unroll
  for (int k1 = 0; k1 < 8; ++k1) slab[wf5_x1(k1, hi, lo)] = A[k1];  // source: n2 = t >> 3, n3 = t & 7
  wf_sync();
  wf2 B[8];
#pragma unroll
  for (int n2 = 0; n2 < 8; ++n2) B[n2] = slab[wf5_x1(lo, n2, hi)];  // dest: k1 = t & 7, n3 = t >> 3
  wf_sync();
  wf_dft8(B);
#pragma unroll
  for (int k2 = 1; k2 < 8; ++k2) B[k2] = wf_cmul(B[k2], twB[hi * 7 + k2 - 1]);
#pragma unroll
  for (int k2 = 0; k2 < 8; ++k2) slab[wf5_x2(k2, hi, lo)] = B[k2];
  wf_sync();
  wf2 e[4], o[4], z[8];
#pragma unroll
  for (int n3 = 0; n3 < 8; ++n3) {  // dest: c = t = k1 + 8 k2
    const wf2 v = slab[wf5_x2(hi, n3, lo)];
    if (n3 & 1) o[n3 >> 1] = v; else e[n3 >> 1] = v;
  }
  wf_sync();
  wf_dft8_pruned<2>(e, o, z);
  // bin 512 - k lives in lane (64 - t) & 63 at 7 - k3 (lane 0: itself at (8 - k3) & 7)
  const int p = (64 - t) & 63;
  const wf2 zp7 = wf2{__shfl(z[7].x, p), __shfl(z[7].y, p)};
  const wf2 zp6 = wf2{__shfl(z[6].x, p), __shfl(z[6].y, p)};
  const wf2 m0 = t == 0 ? z[0] : zp7, m1 = t == 0 ? zp7 : zp6;
  X[0] = wf_unpack(z[0], m0, twK[t]);
  X[1] = wf_unpack(z[1], m1, twK[t + 64]);
}

// RAW (N2): 1 = u8, 2 = i16 patch rows conditioned on the fly, A = (raw * gain - job_sub[job]) * mean_rstd[1]
// * mask^e.  A patch job's gain sits at its offset within its frame: gain + job_off[job] % frame_area, with the
// frames' row pitch (the gain pair of a lane is one 8-byte load next to its 2- / 4-byte raw pair).
// the two raw samples of a lane as loaded (u8: 2 bytes, i16: 4 bytes; one register until they are widened)
template <int RAW>
__device__ __forceinline__ unsigned wf5_ld2raw(const void* row, int x) {
  if constexpr (RAW == 1) {
    unsigned short v;
    __builtin_memcpy(&v, static_cast<const unsigned char*>(row) + x, 2);
    return v;
  } else {
    unsigned v;
    __builtin_memcpy(&v, static_cast<const short*>(row) + x, 4);
    return v;
  }
}
template <int RAW>
__device__ __forceinline__ wf2 wf5_widen2raw(unsigned v) {
  if constexpr (RAW == 1) return wf2{(float)(v & 0xffu), (float)(v >> 8)};
  else return wf2{(float)(short)(v & 0xffffu), (float)((int)v >> 16)};
}

// (raw DUAL: the gain pairs next to the raw and mask ones need a few registers more than five waves per SIMD
// leave, so it aims at four rather than spill)
template <bool DUAL, bool HALF, int RAW = 0>
__global__ __launch_bounds__(256, (RAW && DUAL) ? 4 : WF5_MIN_WAVES) void xc_rows_fwd_wave512(
    const void* __restrict__ src_any, const int64_t* __restrict__ job_off, int64_t row_stride,
    const int* __restrict__ expo_a, const int* __restrict__ expo_b, const float* __restrict__ mask,
    const float* __restrict__ mean_rstd, cfloat* __restrict__ T1a, cfloat* __restrict__ T1b,
    const cfloat* __restrict__ tw_row, XcGeom g, const int2* __restrict__ chord,
    const float* __restrict__ gain, int64_t frame_area, const float* __restrict__ job_sub) {
  __shared__ __attribute__((aligned(16))) wf2 slabs[4][WF5_SLAB];
  __shared__ __attribute__((aligned(16))) wf2 tab[WF5_TWA + WF5_TWB + WF5_TWK];
  const wf2* twA = tab;
  const wf2* twB = tab + WF5_TWA;
  const wf2* twK = tab + WF5_TWA + WF5_TWB;
  const int t = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  wf2* slab = slabs[wv];
  const int job = blockIdx.x, grp = blockIdx.y;
  {  // tables from tw_row[k] = exp(-2 pi i k / 1024): W_512^m = tw_row[2 m], W_64^m = tw_row[16 m]
    constexpr int NTAB = WF5_TWA + WF5_TWB + WF5_TWK, PER = (NTAB + 255) / 256;
    cfloat tv[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      int i = threadIdx.x + 256 * j;
      i = i < NTAB ? i : NTAB - 1;
      int src_k;
      if (i < WF5_TWA) src_k = 2 * (i & 63) * ((i >> 6) + 1);
      else if (i < WF5_TWA + WF5_TWB) src_k = 16 * ((i - WF5_TWA) / 7) * ((i - WF5_TWA) % 7 + 1);
      else src_k = i - WF5_TWA - WF5_TWB;
      tv[j] = tw_row[src_k];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = threadIdx.x + 256 * j;
      if (i < NTAB) tab[i] = wf_from(tv[j]);
    }
  }
  const float mean = RAW ? job_sub[job] : (mean_rstd ? mean_rstd[0] : 0.f);
  const float rstd = mean_rstd ? mean_rstd[1] : 1.f;
  const int ea = expo_a[job], eb = DUAL ? expo_b[job] : 1;
  const float* base = (HALF || RAW) ? nullptr : static_cast<const float*>(src_any) + job_off[job];
  const _Float16* base_h = HALF ? static_cast<const _Float16*>(src_any) + job_off[job] : nullptr;
  const char* base_r = RAW ? static_cast<const char*>(src_any) + job_off[job] * (RAW == 1 ? 1 : 2) : nullptr;
  const float* gbase = RAW ? gain + job_off[job] % frame_area : nullptr;
  cfloat* outa = T1a + (int64_t)job * g.nkx * g.ny;
  cfloat* outb = DUAL ? T1b + (int64_t)job * g.nkx * g.ny : nullptr;
  const int r16 = grp * WF5_ROWS_PER_WG;
  const int rounds = min(WF5_ROWS_PER_WG / 8, (g.ny - r16) / 8);  // ny % 8 == 0
  const int nrows = rounds > 0 ? 2 * rounds : 0;
  const int bxlo = g.x0, bxhi = g.x1 - 2;  // both even: a pair of samples is in or out as a whole
  __syncthreads();
  wf2 Xae[2], Xbe[2];  // bins of the even row of the current pair
#pragma unroll 1
  for (int rr = 0; rr < nrows; ++rr) {
    const int r = r16 + (rr >> 1) * 8 + 2 * wv + (rr & 1);
    const int y = g.y0 + r;
    // with a chord table: only this row's chord of the mask disk is fetched (21 % fewer samples)
    const int xlo = chord ? chord[y].x : bxlo, xhi = chord ? chord[y].y + 2 : bxhi;
    int tl = t;
    asm volatile("" : "+v"(tl));  // per-row addresses are re-derived, not carried (registers)
    const float* row = (HALF || RAW) ? nullptr : base + (int64_t)y * row_stride;
    const _Float16* row_h = HALF ? base_h + (int64_t)y * row_stride : nullptr;
    const char* row_r = RAW ? base_r + (int64_t)y * row_stride * (RAW == 1 ? 1 : 2) : nullptr;
    const float* grow = RAW ? gbase + (int64_t)y * row_stride : nullptr;
    const float* mrow = mask + (int64_t)y * g.W;
    wf2 A[8], Bv[8], mk[8];
    if constexpr (RAW != 0) {
      unsigned rv[8];
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1) {  // raw, gain and mask loads all in flight before anything is used
        const int x = 128 * n1 + 2 * tl;
        const int xc = min(max(x, xlo), xhi);  // outside the support: mask == 0
        rv[n1] = wf5_ld2raw<RAW>(row_r, xc);
        A[n1] = wf5_ld2(grow + xc);  // the gain pair, multiplied in place below
        mk[n1] = *reinterpret_cast<const wf2*>(mrow + x);
      }
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1)
        A[n1] = __builtin_elementwise_fma(wf5_widen2raw<RAW>(rv[n1]), A[n1], wf2{-mean, -mean}) * rstd;
    } else {
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1) {  // all sixteen loads in flight before anything is used
        const int x = 128 * n1 + 2 * tl;
        const int xc = min(max(x, xlo), xhi);  // outside the support: mask == 0
        A[n1] = HALF ? wf5_ld2h(row_h + xc) : wf5_ld2(row + xc);
        mk[n1] = *reinterpret_cast<const wf2*>(mrow + x);
      }
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1) A[n1] = (A[n1] - mean) * rstd;
    }
    if (DUAL && ea == 1 && eb == 2) {  // the leave-one-out schedule's only pair: mask and mask^2, no power loop
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1) {
        A[n1] = A[n1] * mk[n1];
        Bv[n1] = A[n1] * mk[n1];
      }
    } else {  // mask^ea and mask^eb: wave-uniform trip counts, kept out of the load loop
      wf2 pw[8];
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1) pw[n1] = mk[n1];
      for (int e = 1; e < (DUAL ? eb : ea); ++e) {
#pragma unroll
        for (int n1 = 0; n1 < 8; ++n1) pw[n1] *= mk[n1];
      }
      if (DUAL) {
#pragma unroll
        for (int n1 = 0; n1 < 8; ++n1) Bv[n1] = A[n1] * pw[n1];
#pragma unroll
        for (int n1 = 0; n1 < 8; ++n1) pw[n1] = mk[n1];
        for (int e = 1; e < ea; ++e) {
#pragma unroll
          for (int n1 = 0; n1 < 8; ++n1) pw[n1] *= mk[n1];
        }
      }
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1) A[n1] = A[n1] * pw[n1];
    }
    wf2 Xa[2], Xb[2];
    wf5_fft(A, tl, slab, twA, twB, twK, Xa);
    if (DUAL) wf5_fft(Bv, tl, slab, twA, twB, twK, Xb);
    if (rr & 1) {
      float4* park = reinterpret_cast<float4*>(slab);  // [spectrum][128 kx] = {even row, odd row}
      park[tl] = make_float4(Xae[0].x, Xae[0].y, Xa[0].x, Xa[0].y);
      park[tl + 64] = make_float4(Xae[1].x, Xae[1].y, Xa[1].x, Xa[1].y);
      if (DUAL) {
        park[128 + tl] = make_float4(Xbe[0].x, Xbe[0].y, Xb[0].x, Xb[0].y);
        park[128 + tl + 64] = make_float4(Xbe[1].x, Xbe[1].y, Xb[1].x, Xb[1].y);
      }
      __syncthreads();
      {
        const int r8 = r16 + (rr >> 1) * 8;
        const float4* parked = reinterpret_cast<const float4*>(&slabs[0][0]);
        const int per = 4 * g.nkx;  // 4 lanes = the 64 bytes (8 rows) of one kx
        for (int j = threadIdx.x; j < (DUAL ? 2 : 1) * per; j += 256) {
          const int sp = j >= per, jj = j - sp * per;
          const int kx = jj >> 2, w = jj & 3;
          cfloat* out = sp ? outb : outa;
          *reinterpret_cast<float4*>(out + (int64_t)kx * g.ny + r8 + 2 * w) =
              parked[w * (WF5_SLAB / 2) + sp * 128 + kx];
        }
      }
      __syncthreads();
    } else {
      Xae[0] = Xa[0]; Xae[1] = Xa[1];
      if (DUAL) { Xbe[0] = Xb[0]; Xbe[1] = Xb[1]; }
    }
  }
}

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

// go(A, B) with std::bool_constant tags of two runtime choices (as mc_pick in mc_common.h), so that exactly
// the combinations an entry point can reach are instantiated
template <class Go>
static void xc_pick2(bool a, bool b, Go&& go) {
  if (a && b) go(std::true_type{}, std::true_type{});
  else if (a) go(std::true_type{}, std::false_type{});
  else if (b) go(std::false_type{}, std::true_type{});
  else go(std::false_type{}, std::false_type{});
}

// Rows the wave-per-row engine can transform: 4096 samples, at most 512 kept bins, whole rounds of 8 rows
static bool wave_rows_shape(const XcGeom& g) { return g.W == 2 * WF_N && g.nkx <= 512 && (g.ny % 8) == 0; }
static dim3 wave_rows_grid(const XcGeom& g, int njobs) {  // linear id = x + gridDim.x * y, decoded in the kernel
  const int ngroups = (g.ny + WF_ROWS_PER_WG - 1) / WF_ROWS_PER_WG;
  return dim3((ngroups + 7) / 8 * 8, njobs);
}
// ... and the fp32 / fp16 jobs it takes: one mask, no per-job exponent, a statistics box of whole 256-sample
// chunks.  It reads samples and mask rows with 16-byte loads; job_off[] lives on the device: callers of the
// C ABI keep it a multiple of 4 floats whenever W == 4096 (whole frames: f * h * w; documented in mcorr.h).
static bool wave_rows_take(const XcGeom& g, const void* src, const float* mask, const int* job_expo,
                           int64_t row_stride, const XcBox& b, bool stats) {
  const bool aligned =
      ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(mask)) & 15) == 0 && (row_stride & 3) == 0;
  return wave_rows_shape(g) && mask && !job_expo && aligned && (!stats || ((b.wl | b.wu) & 255) == 0);
}

// The workgroup-per-row engine: any power-of-two width
using RowsFwdKernel = decltype(&xc_rows_fwd<4, false, 0>);
template <bool STATS, int RAW>
static int rows_fwd_kernel(int logn, RowsFwdKernel* k) {
  MC_DISPATCH_LOG(logn, *k = xc_rows_fwd<L, STATS, RAW>);
  return MC_OK;
}
static int rows_fwd_wg_launch(RowsFwdKernel k, const void* src, const int64_t* job_off, int64_t row_stride,
                              const int* job_expo, const float* mask, const float* mean_rstd, void* T1,
                              const void* tw_row, int njobs, const XcGeom& g, const XcBox& b, double* stats_acc,
                              const float* gain, const float* job_sub, void* stream) {
  const size_t lds = rows_lds_bytes(g.W / 2, g);
  const int rc = mc_dyn_lds(k, lds);
  if (rc) return rc;
  hipLaunchKernelGGL(k, dim3(njobs, g.ny / g.RG), dim3(MC_WG), lds, (hipStream_t)stream, src, job_off, row_stride,
                     job_expo, mask, mean_rstd, (cfloat*)T1, (const cfloat*)tw_row, g, b, stats_acc, gain, job_sub);
  return mc_check_launch();
}

// the wave-per-1024-sample-row engine: patch rows in any storage, one or two mask exponents per job
template <class Pick>
static int rows_forward_dual_launch(Pick&& pick, const void* src, const int64_t* job_off, int64_t row_stride,
                                    const int* expo_a, const int* expo_b, const float* mask, const float* mean_rstd,
                                    void* T1a, void* T1b, const void* tw_row, int njobs, const XcGeom& g,
                                    const int* row_chord, const float* gain, int64_t frame_area,
                                    const float* job_sub, void* stream) {
  const dim3 grid(njobs, (g.ny + WF5_ROWS_PER_WG - 1) / WF5_ROWS_PER_WG);
  pick([&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, src, job_off, row_stride, expo_a, expo_b, mask,
                       mean_rstd, (cfloat*)T1a, expo_b ? (cfloat*)T1b : (cfloat*)nullptr, (const cfloat*)tw_row, g,
                       (const int2*)row_chord, gain, frame_area, job_sub);
  });
  return mc_check_launch();
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
  const bool wave = wave_rows_take(g, src, mask, job_expo, row_stride, b, stats_acc != nullptr);
  // fp16 samples: only the wave-per-row engine reads them (4096-column frames); anything else is
  // MC_ERR_UNSUPPORTED and the caller widens the stack once
  if (half && !wave) return MC_ERR_UNSUPPORTED;
  if (!wave || g_row_engine == 1) {
    RowsFwdKernel k;
    rc = stats_acc ? rows_fwd_kernel<true, 0>(mc_ilog2(g.W) - 1, &k) : rows_fwd_kernel<false, 0>(mc_ilog2(g.W) - 1, &k);
    if (rc) return rc;
    return rows_fwd_wg_launch(k, src, job_off, row_stride, job_expo, mask, mean_rstd, T1, tw_row, njobs, g, b,
                              stats_acc, nullptr, nullptr, stream);
  }
  // Whole 128-byte lines of T1 (16 rows per kx) when the first round's bins fit next to the slabs with two
  // workgroups per CU still resident, and every 16-row piece is line-aligned.  OFF: it saves the 0.15 GB of
  // write amplification (one stream: 2.00 -> 1.97 ms per 40 x 4096^2 step) but its 26 KB of extra LDS per
  // workgroup keeps the warp's tiles of the other stream out of the CU: 1.74 -> 1.84 ms per step under the
  // two-stream overlap.  It also needs WF_ROWS_PER_WG == 16.
  constexpr bool K1_LINES16 = false;
  const size_t park_bytes = (size_t)4 * g.nkx * 16;
  const int lines16 = K1_LINES16 && WF_ROWS_PER_WG == 16 && (g.ny % 16) == 0 && park_bytes <= 27 * 1024 &&
                      (reinterpret_cast<uintptr_t>(T1) & 127) == 0;
  const size_t dyn = lines16 ? park_bytes : 0;
  auto launch = [&](auto kernel) {
    if (dyn) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    hipLaunchKernelGGL(kernel, wave_rows_grid(g, njobs), dim3(256), dyn, (hipStream_t)stream, (const void*)src,
                       job_off, row_stride, mask, mean_rstd, (cfloat*)T1, (const cfloat*)tw_row, g, b, stats_acc,
                       (const int2*)row_chord, lines16, (const float*)nullptr, (const float*)nullptr);
  };
  // square 4096 frames: the first and the last 256-sample chunk of a row lie outside the mask's support
  const bool inner = g.x0 >= 256 && g.x0 <= 512 && g.x1 >= 3584 && g.x1 <= 3840;
  xc_pick2(g.nkx <= 256, stats_acc != nullptr, [&](auto keep1, auto stats) {
    constexpr int KEEP = decltype(keep1)::value ? 1 : 2;
    constexpr bool ST = decltype(stats)::value;
    // fp16 storage: the general variant (all 16 chunks, per-row chord clamp when given)
    if (half) launch(xc_rows_fwd_wave<KEEP, ST, 0, 16, true, true>);
    else if (inner && row_chord) launch(xc_rows_fwd_wave<KEEP, ST, 1, 15, true>);  // per-row chord clamp
    else if (inner) launch(xc_rows_fwd_wave<KEEP, ST, 1, 15, false>);
    else launch(xc_rows_fwd_wave<KEEP, ST, 0, 16, true>);
  });
  return mc_check_launch();
}

int mc_xc_rows_forward_dual(const float* src, const int64_t* job_off, int64_t row_stride,
                            const int* expo_a, const int* expo_b, const float* mask,
                            const float* mean_rstd, void* T1a, void* T1b, const void* tw_row,
                            int njobs, const mc_xc_geom* q, const int* row_chord, void* stream) {
  return mc_xc_rows_forward_dual_t(src, MC_STORE_F32, job_off, row_stride, expo_a, expo_b, mask, mean_rstd,
                                   T1a, T1b, tw_row, njobs, q, row_chord, stream);
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
  if (g.W != 2 * WF5_N || g.nkx > 128 || (g.ny % 8) || (reinterpret_cast<uintptr_t>(mask) & 7))
    return MC_ERR_UNSUPPORTED;
  auto pick = [&](auto launch) {
    xc_pick2(expo_b != nullptr, storage == MC_STORE_F16, [&](auto dual, auto half) {
      launch(xc_rows_fwd_wave512<decltype(dual)::value, decltype(half)::value>);
    });
  };
  return rows_forward_dual_launch(pick, src, job_off, row_stride, expo_a, expo_b, mask, mean_rstd, T1a, T1b, tw_row,
                                  njobs, g, row_chord, nullptr, 1, nullptr, stream);
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
  if (g.W != 2 * WF5_N || g.nkx > 128 || (g.ny % 8) || (reinterpret_cast<uintptr_t>(mask) & 7) ||
      (reinterpret_cast<uintptr_t>(gain) & 3) || (storage == MC_STORE_I16 && (reinterpret_cast<uintptr_t>(raw) & 1)))
    return MC_ERR_UNSUPPORTED;
  auto pick = [&](auto launch) {
    xc_pick2(expo_b != nullptr, storage == MC_STORE_U8, [&](auto dual, auto u8) {
      launch(xc_rows_fwd_wave512<decltype(dual)::value, false, decltype(u8)::value ? 1 : 2>);
    });
  };
  return rows_forward_dual_launch(pick, raw, job_off, row_stride, expo_a, expo_b, mask, mean_rstd, T1a, T1b, tw_row,
                                  njobs, g, row_chord, gain, frame_area, job_sub, stream);
}

int mc_xc_rows_forward(const float* src, const int64_t* job_off, int64_t row_stride,
                       const int* job_expo, const float* mask, const float* mean_rstd,
                       void* T1, const void* tw_row, int njobs, const mc_xc_geom* q,
                       void* stream) {
  return rows_forward_impl(src, job_off, row_stride, job_expo, mask, mean_rstd, T1, tw_row, njobs, q,
                           nullptr, nullptr, stream);
}

int mc_xc_provisional_mean(const float* x, int n, float* m0, void* stream) {
  if (!x || !m0 || n < 1) return MC_ERR_ARG;
  hipLaunchKernelGGL(xc_provisional_mean_kernel<float>, dim3(1), dim3(256), 0, (hipStream_t)stream, x, n, m0);
  return mc_check_launch();
}

int mc_xc_provisional_mean_t(const void* x, int storage, int n, float* m0, void* stream) {
  if (!x || !m0 || n < 1) return MC_ERR_ARG;
  if (storage == MC_STORE_F32) return mc_xc_provisional_mean(static_cast<const float*>(x), n, m0, stream);
  if (storage != MC_STORE_F16) return MC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(xc_provisional_mean_kernel<_Float16>, dim3(1), dim3(256), 0, (hipStream_t)stream,
                     static_cast<const _Float16*>(x), n, m0);
  return mc_check_launch();
}

int mc_xc_rows_forward_stats(const float* src, const int64_t* job_off, int64_t row_stride,
                             const float* mask, const float* m0, void* T1, const void* tw_row,
                             int njobs, const mc_xc_geom* q, int hl, int hu, int wl, int wu,
                             double* acc, float* fix, float* out3, const int* row_chord, void* stream) {
  return mc_xc_rows_forward_stats_t(src, MC_STORE_F32, job_off, row_stride, mask, m0, T1, tw_row, njobs, q, hl, hu,
                                    wl, wu, acc, fix, out3, row_chord, stream);
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
  const uintptr_t al = reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(gain) |
                       reinterpret_cast<uintptr_t>(mask);
  const bool u8 = storage == MC_STORE_U8;
  const XcBox b{0, 0, 0, 0};
  if (!(wave_rows_shape(g) && (al & 15) == 0 && (row_stride & 7) == 0)) {
    // any other power-of-two width: the workgroup-per-row engine, element-wise loads of raw and gain
    RowsFwdKernel k;
    rc = u8 ? rows_fwd_kernel<false, 1>(mc_ilog2(g.W) - 1, &k) : rows_fwd_kernel<false, 2>(mc_ilog2(g.W) - 1, &k);
    if (rc) return rc;
    return rows_fwd_wg_launch(k, raw, job_off, row_stride, nullptr, mask, mean_rstd, T1, tw_row, njobs, g, b, nullptr,
                              gain, job_sub, stream);
  }
  xc_pick2(g.nkx <= 256, u8, [&](auto keep1, auto is_u8) {
    hipLaunchKernelGGL((xc_rows_fwd_wave<decltype(keep1)::value ? 1 : 2, false, 0, 16, true, false,
                                         decltype(is_u8)::value ? 1 : 2>),
                       wave_rows_grid(g, njobs), dim3(256), 0, (hipStream_t)stream, raw, job_off, row_stride, mask,
                       mean_rstd, (cfloat*)T1, (const cfloat*)tw_row, g, b, (double*)nullptr, (const int2*)row_chord, 0,
                       gain, job_sub);
  });
  return mc_check_launch();
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
