// K1 of the pruned cross-correlation engine (xc_common.h has the map of the passes), the workgroup-per-row engine:
// a workgroup per row group, any power-of-two width, fp32 / u8 / i16 samples.  xc_rows_fwd.hip has the entry
// points and the rule that routes a job here.
#include "xc_rows_fwd.h"

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

// ------------------------------------------------------------------ host side
using RowsFwdKernel = decltype(&xc_rows_fwd<4, false, 0>);
template <bool STATS, int RAW>
static int rows_fwd_kernel(int logn, RowsFwdKernel* k) {
  MC_DISPATCH_LOG(logn, *k = xc_rows_fwd<L, STATS, RAW>);
  return MC_OK;
}
int k1_wg_launch(int raw, const void* src, const int64_t* job_off, int64_t row_stride, const int* job_expo,
                 const float* mask, const float* mean_rstd, void* T1, const void* tw_row, int njobs, const XcGeom& g,
                 const XcBox& b, double* stats_acc, const float* gain, const float* job_sub, void* stream) {
  RowsFwdKernel k;
  const int logn = mc_ilog2(g.W) - 1;
  int rc = raw == 1 ? rows_fwd_kernel<false, 1>(logn, &k) : raw == 2 ? rows_fwd_kernel<false, 2>(logn, &k)
           : stats_acc ? rows_fwd_kernel<true, 0>(logn, &k) : rows_fwd_kernel<false, 0>(logn, &k);
  if (rc) return rc;
  const size_t lds = rows_lds_bytes(g.W / 2, g);
  rc = mc_dyn_lds(k, lds);
  if (rc) return rc;
  hipLaunchKernelGGL(k, dim3(njobs, g.ny / g.RG), dim3(MC_WG), lds, (hipStream_t)stream, src, job_off, row_stride,
                     job_expo, mask, mean_rstd, (cfloat*)T1, (const cfloat*)tw_row, g, b, stats_acc, gain, job_sub);
  return mc_check_launch();
}
