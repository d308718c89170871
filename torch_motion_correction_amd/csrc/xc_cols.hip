// K2 and K3 of the pruned cross-correlation engine (xc_common.h has the map of the passes): the forward and
// inverse column transforms, by three engines each -- radix-8 Stockham lines (any power-of-two height), the
// register-resident radix-16 transform (4096) and a wavefront per column (1024).  The choice between them is
// made here only; mc_xc_correlate_argmax (xc_search.hip) reaches its column passes through mc_launch_cols_*.
#include "xc_common.h"

// ------------------------------------------------------------------ K2: columns forward
// fix (optional): {dmean, rstd} and Mhat = pruned spectrum of the mask: the spectrum of
// ((x - m0) - dmean) * rstd * mask is (Y - dmean * Mhat) * rstd by linearity.
constexpr int XC_FWD_COLS = 2;  // columns per workgroup in the radix-16 K2, the second one fetched under the first (1: 107, 2: 101, 4: 105 us)
// R16 (H = 4096, kyp and kyn <= 512): the register-resident radix-16 transform of mc_fft.h
// with the unwanted output rows pruned at compile time.
template <int LOGH, bool R16 = false>
__global__ __launch_bounds__(MC_WG) void xc_cols_fwd(const cfloat* __restrict__ T1,
                                                     const float* __restrict__ filt,
                                                     cfloat* __restrict__ S,
                                                     const cfloat* __restrict__ tw_col, XcGeom g,
                                                     const float* __restrict__ fix,
                                                     const cfloat* __restrict__ Mhat) {
  constexpr int H = 1 << LOGH;
  __shared__ __attribute__((aligned(16))) cfloat line[R16 ? H : lds_len(H)];  // radix 16: unpadded, 5 workgroups / CU
  const int tid = threadIdx.x;
  const int kx = blockIdx.x, job = blockIdx.y;
  const cfloat* col = T1 + ((int64_t)job * g.nkx + kx) * g.ny;
  const int nky = g.kyp + g.kyn;
  cfloat* out = S + ((int64_t)job * g.nkx + kx) * nky;
  const float* f = filt ? filt + (int64_t)kx * nky : nullptr;
  const cfloat* mh = fix ? Mhat + (int64_t)kx * nky : nullptr;
  const float dmean = fix ? fix[0] : 0.f, rstd = fix ? fix[1] : 1.f;
  auto load = [&](int y) {
    const int yy = y - g.y0;
    return (yy >= 0 && yy < g.ny) ? col[yy] : cmake(0.f, 0.f);
  };
  auto store = [&](int ky, cfloat v) {
    int kyi = -1;
    if (ky < g.kyp) kyi = ky;
    else if (ky >= H - g.kyn) kyi = ky - (H - g.kyn) + g.kyp;
    if (kyi >= 0) {
      if (fix) {
        const cfloat m = mh[kyi];
        v = cmake((v.x - dmean * m.x) * rstd, (v.y - dmean * m.y) * rstd);
      }
      out[kyi] = f ? cscale(v, f[kyi]) : v;
    }
  };
  if constexpr (R16) {
    // XC_FWD_COLS consecutive kx columns per workgroup (blockIdx.x counts column groups): the next
    // column's samples are in flight (registers) while the current one is transformed
    const int kx0 = blockIdx.x * XC_FWD_COLS;
    auto fetch = [&](int kxc, cfloat (&v)[16], int tq) {
      const cfloat* c = T1 + ((int64_t)job * g.nkx + kxc) * g.ny;
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) {
        const int yy = 256 * n1 + tq - g.y0;
        v[n1] = (yy >= 0 && yy < g.ny) ? c[yy] : cmake(0.f, 0.f);
      }
    };
    cfloat curv[16], nxtv[16];
    fetch(kx0 < g.nkx ? kx0 : g.nkx - 1, curv, tid);
    // twiddle bases and (below) the filter / mask-spectrum values of the 4 rows this thread stores: all issued with
    // the column's samples, instead of waiting for them in the middle and at the end of the transform
    const R16Tw TW = r16_twiddles(tid, tw_col);
    int kyo[4];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) kyo[s4] = kept_index(tid + 256 * (s4 < 2 ? s4 : s4 + 12), H, g.kyp, g.kyn);
#pragma unroll 1
    for (int cc = 0; cc < XC_FWD_COLS; ++cc) {
      const int kxc = kx0 + cc;
      if (kxc >= g.nkx) break;  // workgroup-uniform
      int tcol = tid;  // opaque per column: nothing derived from it is hoisted (registers)
      asm volatile("" : "+v"(tcol));
      if (cc + 1 < XC_FWD_COLS && kxc + 1 < g.nkx) fetch(kxc + 1, nxtv, tcol);
      cfloat* outc = S + ((int64_t)job * g.nkx + kxc) * nky;
      const float* fc = filt ? filt + (int64_t)kxc * nky : nullptr;
      const cfloat* mhc = fix ? Mhat + (int64_t)kxc * nky : nullptr;
      auto loadr = [&](int n1, int) { return curv[n1]; };
      float fpre[4];
      cfloat mpre[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        fpre[s4] = (fc && kyo[s4] >= 0) ? fc[kyo[s4]] : 1.f;
        mpre[s4] = (fix && kyo[s4] >= 0) ? mhc[kyo[s4]] : cmake(0.f, 0.f);
      }
      auto storer = [&](int k3, int, cfloat v) {  // k3 in {0, 1, 14, 15}, a compile-time constant at every call
        const int s4 = k3 < 2 ? k3 : k3 - 12;
        if (kyo[s4] >= 0) {
          if (fix) v = cmake((v.x - dmean * mpre[s4].x) * rstd, (v.y - dmean * mpre[s4].y) * rstd);
          outc[kyo[s4]] = fc ? cscale(v, fpre[s4]) : v;
        }
      };
      wg_fft4096_r16_tw<-1, 8, 2>(line, tcol, TW, loadr, storer);
      __syncthreads();
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) curv[n1] = nxtv[n1];
    }
  } else {
    wg_fft<H, -1>(line, tid, tw_col, 1, load, store);
  }
}

// ------------------------------------------------------------------ K2 / K3, wave per 1024-point column
// Columns of 1024 x 1024 patches (H = 1024, at most 128 kept rows at either end of the
// spectrum): one wavefront per column, four columns per workgroup, the 16 x 8 x 8 transform of
// mc_wave_fft.h (third part) in registers, no workgroup barrier.  The workgroup-per-column
// kernels spend a 1024-point column on 256 threads (4 values each) and 7 barriers.
// K2: only the kept output rows are produced (k3 in {0, 7} of the last radix-8 pass).
// K3: only the kept input rows are fetched (n1 in {0, 1, 14, 15} of the first radix-16 pass);
//     the inverse runs the forward kernel on conjugated data.
constexpr int XC_NEAR_MIN_WAVES = 4;  // register target of the near-window column passes (5: 96 VGPRs, spills)
constexpr int XC_FWDW_COLS = 1;  // columns per wavefront in xc_cols_fwd_wave1024 (4 measured slower: the kernel streams T1 at 3.2 TB/s)
// The six table entries a lane needs (they depend on the lane only): loaded once, up front -- behind the
// acquire fence of wf_sync the compiler cannot start them early, and a wave waited for the L2 in the middle of
// every column.
struct Wf10Tw {
  wf2 w1, w2, w4, w8, b[2];
};
__device__ __forceinline__ Wf10Tw wf10_twiddles(int t, const cfloat* __restrict__ tw) {
  Wf10Tw T;
  T.w1 = wf_from(tw[t]); T.w2 = wf_from(tw[2 * t]); T.w4 = wf_from(tw[4 * t]); T.w8 = wf_from(tw[8 * t]);
  T.b[0] = wf_from(tw[16 * (t >> 4)]);
  T.b[1] = wf_from(tw[16 * ((t >> 4) + 4)]);
  return T;
}
__device__ __forceinline__ void wf10_passes_ab(wf2 (&a)[16], int t, wf2* slab, const Wf10Tw& T,
                                               wf2 (&B)[2][8]) {
  wf_twiddle16(a, T.w1, T.w2, T.w4, T.w8);
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) slab[wf10_x1(k1, t)] = a[k1];
  wf_sync();
  const int k1 = t & 15;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int n3 = (t >> 4) + 4 * b;
#pragma unroll
    for (int n2 = 0; n2 < 8; ++n2) B[b][n2] = slab[wf10_x1(k1, 8 * n2 + n3)];
  }
  wf_sync();
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    wf_dft8(B[b]);
    wf_twiddle8(B[b], T.b[b]);  // W_64^{n3 k2}
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) slab[wf10_x2(k1, k2, (t >> 4) + 4 * b)] = B[b][k2];
  }
  wf_sync();
}

__global__ __launch_bounds__(256) void xc_cols_fwd_wave1024(const cfloat* __restrict__ T1,
                                                            const float* __restrict__ filt,
                                                            cfloat* __restrict__ S,
                                                            const cfloat* __restrict__ tw_col, XcGeom g,
                                                            const float* __restrict__ fix,
                                                            const cfloat* __restrict__ Mhat) {
  constexpr int H = 1024;
  __shared__ __attribute__((aligned(16))) wf2 slabs[4][WF10_N];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kx0 = (blockIdx.x * 4 + wv) * XC_FWDW_COLS, job = blockIdx.y;
  if (kx0 >= g.nkx) return;  // no workgroup barrier below
  wf2* slab = slabs[wv];
  const int nky = g.kyp + g.kyn;
  const float dmean = fix ? fix[0] : 0.f, rstd = fix ? fix[1] : 1.f;
  const Wf10Tw TW = wf10_twiddles(threadIdx.x & 63, tw_col);
  // (a one-trip loop today; written without it the same statements compile to a different schedule, so it stays
  // until a change of this kernel is measured)
#pragma unroll 1
  for (int cc = 0; cc < XC_FWDW_COLS; ++cc) {
  const int kx = kx0 + cc;
  if (kx >= g.nkx) break;  // wave-uniform
  int tq = threadIdx.x & 63;  // opaque per column: nothing derived from it is hoisted (registers)
  asm volatile("" : "+v"(tq));
  const int t = tq;
  const cfloat* col = T1 + ((int64_t)job * g.nkx + kx) * g.ny;
  cfloat* out = S + ((int64_t)job * g.nkx + kx) * nky;
  const float* f = filt ? filt + (int64_t)kx * nky : nullptr;
  const cfloat* mh = fix ? Mhat + (int64_t)kx * nky : nullptr;
  wf2 a[16], B[2][8];
#pragma unroll
  for (int n1 = 0; n1 < 16; ++n1) {
    const int yy = 64 * n1 + t - g.y0;
    a[n1] = (yy >= 0 && yy < g.ny) ? wf_from(col[yy]) : wf2{0.f, 0.f};
  }
  // filter and mask-spectrum values of the (at most four) rows this lane stores: fetched with the samples
  int kyo[2][2];
  float fpre[2][2];
  cfloat mpre[2][2];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int sel = 0; sel < 2; ++sel) {
      const int ky = (t & 15) + 16 * ((t >> 4) + 4 * b) + (sel ? 896 : 0);
      int kyi = -1;
      if (ky < g.kyp) kyi = ky;
      else if (ky >= H - g.kyn) kyi = ky - (H - g.kyn) + g.kyp;
      kyo[b][sel] = kyi;
      fpre[b][sel] = (f && kyi >= 0) ? f[kyi] : 1.f;
      mpre[b][sel] = (fix && kyi >= 0) ? mh[kyi] : cmake(0.f, 0.f);
    }
  wf_dft16(a);
  wf10_passes_ab(a, t, slab, TW, B);
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int k1 = t & 15, k2 = (t >> 4) + 4 * b;
    wf2 e[4], o[4], z[8];
#pragma unroll
    for (int n3 = 0; n3 < 8; ++n3) {
      const wf2 v = slab[wf10_x2(k1, k2, n3)];
      if (n3 & 1) o[n3 >> 1] = v; else e[n3 >> 1] = v;
    }
    wf_sync();
    wf_dft8_pruned<1>(e, o, z);  // k3 = 0 and 7
#pragma unroll
    for (int sel = 0; sel < 2; ++sel) {
      const int kyi = kyo[b][sel];
      if (kyi >= 0) {
        cfloat v = wf_to(z[sel ? 7 : 0]);
        if (fix) v = cmake((v.x - dmean * mpre[b][sel].x) * rstd, (v.y - dmean * mpre[b][sel].y) * rstd);
        out[kyi] = f ? cscale(v, fpre[b][sel]) : v;
      }
    }
  }
  }
}

__global__ __launch_bounds__(256) void xc_cols_inv_wave1024(
    const cfloat* __restrict__ S_cur, const int* __restrict__ cur_idx,
    const cfloat* __restrict__ S_ref, const int* __restrict__ ref_idx, cfloat* __restrict__ T2,
    const cfloat* __restrict__ tw_col, float scale, XcGeom g) {
  constexpr int H = 1024;
  __shared__ __attribute__((aligned(16))) wf2 slabs[4][WF10_N];
  const int t = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kx = blockIdx.x * 4 + wv, p = blockIdx.y;
  if (kx >= g.nkx) return;  // no workgroup barrier below
  wf2* slab = slabs[wv];
  const int nky = g.kyp + g.kyn;
  const cfloat* cur = S_cur + ((int64_t)cur_idx[p] * g.nkx + kx) * nky;
  const cfloat* ref = S_ref + ((int64_t)ref_idx[p] * g.nkx + kx) * nky;
  cfloat* out = T2 + ((int64_t)p * g.nkx + kx) * H;
  wf2 a[16], B[2][8];
#pragma unroll
  for (int n1 = 0; n1 < 16; ++n1) {
    a[n1] = wf2{0.f, 0.f};
    if (n1 < 2 || n1 >= 14) {  // the only input rows a band-limited spectrum can hold
      const int kyi = kept_index(64 * n1 + t, H, g.kyp, g.kyn);
      if (kyi >= 0) {
        const cfloat v = cscale(cmulc(ref[kyi], cur[kyi]), scale);
        a[n1] = wf2{v.x, -v.y};  // conjugate in, conjugate out: inverse transform
      }
    }
  }
  const Wf10Tw TW = wf10_twiddles(t, tw_col);
  wf_dft16(a);
  wf10_passes_ab(a, t, slab, TW, B);
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int k1 = t & 15, k2 = (t >> 4) + 4 * b;
    wf2 c[8];
#pragma unroll
    for (int n3 = 0; n3 < 8; ++n3) c[n3] = slab[wf10_x2(k1, k2, n3)];
    wf_dft8(c);
#pragma unroll
    for (int k3 = 0; k3 < 8; ++k3) out[k1 + 16 * k2 + 128 * k3] = cmake(c[k3].x, -c[k3].y);
  }
}

// Near-window form of the same (see xc_cols_inv_near below): a wavefront runs XC_NEAR_COLS
// columns of one pair, keeps the stored window's rows and its share of the row bounds (16 rows
// per lane, in registers over the column loop).
#define XC_NEAR_COLS_W 8
__global__ __launch_bounds__(256, XC_NEAR_MIN_WAVES) void xc_cols_inv_near_wave1024(
    const cfloat* __restrict__ S_cur, const int* __restrict__ cur_idx,
    const cfloat* __restrict__ S_ref, const int* __restrict__ ref_idx, cfloat* __restrict__ T2n,
    float* __restrict__ bounds, const cfloat* __restrict__ tw_col, float scale, XcGeom g, int nstore) {
  constexpr int H = 1024;
  __shared__ __attribute__((aligned(16))) wf2 slabs[4][WF10_N];
  const int t = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = blockIdx.y;
  const int kx0 = (blockIdx.x * 4 + wv) * XC_NEAR_COLS_W;
  if (kx0 >= g.nkx) return;  // no workgroup barrier below
  wf2* slab = slabs[wv];
  const int nky = g.kyp + g.kyn;
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  // twiddles once per wave; a column's eight input values are fetched while the previous column is
  // transformed (as xc_cols_inv_near does: the kernel waited, exposed, at the head of every column)
  const Wf10Tw TW = wf10_twiddles(t, tw_col);
  const int64_t cur_base = (int64_t)cur_idx[p] * g.nkx, ref_base = (int64_t)ref_idx[p] * g.nkx;
  int kyi4[4];
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) kyi4[s4] = kept_index(64 * (s4 < 2 ? s4 : s4 + 12) + t, H, g.kyp, g.kyn);
  cfloat pc[4], pr[4];
  auto fetch4 = [&](int kx, cfloat (&c4)[4], cfloat (&r4)[4]) {
    const cfloat* cur = S_cur + (cur_base + kx) * nky;
    const cfloat* ref = S_ref + (ref_base + kx) * nky;
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      c4[s4] = kyi4[s4] >= 0 ? cur[kyi4[s4]] : cmake(0.f, 0.f);
      r4[s4] = kyi4[s4] >= 0 ? ref[kyi4[s4]] : cmake(0.f, 0.f);
    }
  };
  fetch4(kx0, pc, pr);
#pragma unroll 1
  for (int cc = 0; cc < XC_NEAR_COLS_W; ++cc) {
    const int kx = kx0 + cc;
    if (kx >= g.nkx) break;  // wave-uniform
    int tl = t;  // opaque per column: nothing derived from it is hoisted (registers)
    asm volatile("" : "+v"(tl));
    cfloat* outn = T2n + ((int64_t)p * g.nkx + kx) * (2 * nstore);
    const float wgt = kx == 0 ? 1.f : 2.f;
    wf2 a[16], B[2][8];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {
      a[n1] = wf2{0.f, 0.f};
      if (n1 < 2 || n1 >= 14) {
        const int s4 = n1 < 2 ? n1 : n1 - 12;
        const cfloat v = cscale(cmulc(pr[s4], pc[s4]), scale);  // zero where the row is not kept
        a[n1] = wf2{v.x, -v.y};
      }
    }
    if (cc + 1 < XC_NEAR_COLS_W && kx + 1 < g.nkx) fetch4(kx + 1, pc, pr);
    wf_dft16_lo2(a);  // entries 2..13 are zero
    wf10_passes_ab(a, tl, slab, TW, B);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int k1 = tl & 15, k2 = (tl >> 4) + 4 * b;
      wf2 c[8];
#pragma unroll
      for (int n3 = 0; n3 < 8; ++n3) c[n3] = slab[wf10_x2(k1, k2, n3)];
      wf_sync();
      wf_dft8(c);
#pragma unroll
      for (int k3 = 0; k3 < 8; ++k3) {
        const int y = k1 + 16 * k2 + 128 * k3;
        const int yn = y < nstore ? y : y - (H - 2 * nstore);
        if (yn >= 0 && yn < 2 * nstore && (y < nstore || y >= H - nstore)) outn[yn] = cmake(c[k3].x, -c[k3].y);
        acc[8 * b + k3] += wgt * __builtin_amdgcn_sqrtf(c[k3].x * c[k3].x + c[k3].y * c[k3].y);
      }
    }
  }
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int k3 = 0; k3 < 8; ++k3)
      atomicAdd(&bounds[(int64_t)p * H + (t & 15) + 16 * ((t >> 4) + 4 * b) + 128 * k3], acc[8 * b + k3]);
}

// ------------------------------------------------------------------ K3: columns inverse
// pair p: cur spectrum index cur_idx[p] in S_cur, ref spectrum index ref_idx[p] in S_ref.
// MODE 0: conj(ref)*cur (cross-correlation); MODE 1: cur * phase ramp (Fourier shift,
// correct_motion.py:488-494) -- phase computed in K3 from shifts[p] = (sy, sx).
template <int LOGH, int MODE>
__global__ __launch_bounds__(MC_WG) void xc_cols_inv(
    const cfloat* __restrict__ S_cur, const int* __restrict__ cur_idx,
    const cfloat* __restrict__ S_ref, const int* __restrict__ ref_idx,
    const float* __restrict__ shifts, cfloat* __restrict__ T2, const cfloat* __restrict__ tw_col,
    float scale, XcGeom g, const int* __restrict__ gate) {
  constexpr int H = 1 << LOGH;
  __shared__ __attribute__((aligned(16))) cfloat line[lds_len(H)];
  if (gate && gate[0] == 0) return;  // the near window settled every pair: nothing to do
  const int tid = threadIdx.x;
  const int kx = blockIdx.x, p = blockIdx.y;
  const int nky = g.kyp + g.kyn;
  const cfloat* cur = S_cur + ((int64_t)cur_idx[p] * g.nkx + kx) * nky;
  const cfloat* ref = MODE == 0 ? S_ref + ((int64_t)ref_idx[p] * g.nkx + kx) * nky : nullptr;
  cfloat* out = T2 + ((int64_t)p * g.nkx + kx) * H;
  float sy = 0.f, sx = 0.f, fx = 0.f;
  if (MODE == 1) {
    sy = shifts[2 * p];
    sx = shifts[2 * p + 1];
    fx = (float)kx / (float)g.W;  // rfftfreq
  }
  auto load = [&](int ky) {
    int kyi = -1;
    if (ky < g.kyp) kyi = ky;
    else if (ky >= H - g.kyn) kyi = ky - (H - g.kyn) + g.kyp;
    if (kyi < 0) return cmake(0.f, 0.f);
    cfloat v;
    if (MODE == 0) {
      v = cmulc(ref[kyi], cur[kyi]);
    } else {
      // torch.fft.fftfreq: k/H for k < (H+1)/2 else (k-H)/H; angle = sum(-2*pi*f*s)
      const int kk = (ky < (H + 1) / 2) ? ky : ky - H;
      const float fy = (float)kk / (float)H;
      const float m2pi = -6.283185307179586f;
      const float ang = (m2pi * fy) * sy + (m2pi * fx) * sx;
      float sn, cs;
      sincosf(ang, &sn, &cs);
      v = cmul(cur[kyi], cmake(cs, sn));
    }
    return cscale(v, scale);
  };
  auto store = [&](int y, cfloat v) { out[y] = v; };
  wg_fft<H, +1>(line, tid, tw_col, 1, load, store);
}

// K3 for the arg-max search without the full T2: a workgroup runs XC_NEAR_COLS columns of
// one pair through the inverse column FFT, keeps only the rows of the near window
// (rows [0, nstore) and [H - nstore, H), nstore = near rows + XC_NEAR_GUARD rows for the sub-pixel
// neighbourhood of a peak on the window's edge, xc_search.hip) in T2n[p][kx][2 nstore] and adds
// its share of the triangle-inequality row bounds (see K4) to bounds[p][y] -- per thread in
// registers over its columns, then one float atomic per (thread, row).  The full map is
// only ever materialised (xc_cols_inv, gated by `need_full`) when some far row's bound
// reaches the maximum found in the near window.
constexpr int XC_NEAR_COLS = 8;
template <int LOGH, bool R16 = false>
__global__ __launch_bounds__(MC_WG, XC_NEAR_MIN_WAVES) void xc_cols_inv_near(
    const cfloat* __restrict__ S_cur, const int* __restrict__ cur_idx,
    const cfloat* __restrict__ S_ref, const int* __restrict__ ref_idx, cfloat* __restrict__ T2n,
    float* __restrict__ bounds, const cfloat* __restrict__ tw_col, float scale, XcGeom g, int nstore) {
  constexpr int H = 1 << LOGH;
  __shared__ __attribute__((aligned(16))) cfloat line[R16 ? H : lds_len(H)];
  constexpr int NOUT = H / MC_WG;  // rows per thread in the last pass (H >= 1024: all threads busy)
  const int tid = threadIdx.x;
  const int p = blockIdx.y;
  const int nky = g.kyp + g.kyn;
  // this thread's share of the row bounds: the last pass of every column hands a thread the
  // same NOUT rows in the same order, so the sums stay in registers over the column loop
  float acc[NOUT];
#pragma unroll
  for (int c = 0; c < NOUT; ++c) acc[c] = 0.f;
  const int64_t cur_base = (int64_t)cur_idx[p] * g.nkx, ref_base = (int64_t)ref_idx[p] * g.nkx;
  // R16: a thread's pass-A inputs are rows tid + 256 n1, n1 in {0, 1, 14, 15} (the band-pass keeps |ky| < 512);
  // the next column's eight values are fetched while this column is transformed (its loads used to sit, exposed,
  // at the head of every column: the kernel is neither VALU- nor HBM-bound, profiles/r03_k3n_pmc.txt)
  int kyi4[4];
  cfloat pc[4], pr[4];
  auto fetch4 = [&](int kx, cfloat (&c4)[4], cfloat (&r4)[4]) {
    const cfloat* cur = S_cur + (cur_base + kx) * nky;
    const cfloat* ref = S_ref + (ref_base + kx) * nky;
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      c4[s4] = kyi4[s4] >= 0 ? cur[kyi4[s4]] : cmake(0.f, 0.f);
      r4[s4] = kyi4[s4] >= 0 ? ref[kyi4[s4]] : cmake(0.f, 0.f);
    }
  };
  R16Tw TW;  // twiddle bases: once per workgroup, not eight global loads inside every column
  if constexpr (R16) {
    TW = r16_twiddles(tid, tw_col);
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) kyi4[s4] = kept_index(tid + 256 * (s4 < 2 ? s4 : s4 + 12), H, g.kyp, g.kyn);
    if ((int)blockIdx.x * XC_NEAR_COLS < g.nkx) fetch4(blockIdx.x * XC_NEAR_COLS, pc, pr);
  }
#pragma unroll 1
  for (int cc = 0; cc < XC_NEAR_COLS; ++cc) {
    const int kx = blockIdx.x * XC_NEAR_COLS + cc;
    if (kx >= g.nkx) break;  // workgroup-uniform
    const cfloat* cur = S_cur + (cur_base + kx) * nky;
    const cfloat* ref = S_ref + (ref_base + kx) * nky;
    cfloat* outn = T2n + ((int64_t)p * g.nkx + kx) * (2 * nstore);
    const float wgt = kx == 0 ? 1.f : 2.f;
    auto load = [&](int ky) {
      const int kyi = kept_index(ky, H, g.kyp, g.kyn);
      if (kyi < 0) return cmake(0.f, 0.f);
      return cscale(cmulc(ref[kyi], cur[kyi]), scale);
    };
    cfloat qc[4], qr[4];  // this column's values; pc / pr receive the next column's
    if constexpr (R16) {
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        qc[s4] = pc[s4];
        qr[s4] = pr[s4];
      }
      if (cc + 1 < XC_NEAR_COLS && kx + 1 < g.nkx) fetch4(kx + 1, pc, pr);
    }
    auto load16 = [&](int n1, int) { return cscale(cmulc(qr[n1 < 2 ? n1 : n1 - 12], qc[n1 < 2 ? n1 : n1 - 12]), scale); };
    int c = 0;
    auto store = [&](int y, cfloat v) {
      const int yn = y < nstore ? y : y - (H - 2 * nstore);  // position in the stored window
      if (yn >= 0 && yn < 2 * nstore && (y < nstore || y >= H - nstore)) outn[yn] = v;
      // hardware square root (1 ulp): the bound test carries a 1e-4 relative slack.  (The cheaper upper bound
      // max + (sqrt 2 - 1) min, up to 8 % above |z|, does not make the kernel faster and opens the fall-back on
      // noisier movies: scripts/far_margin.py, noise 4: largest far bound 0.95 of the maximum, 1.001 with it.)
      acc[c++] += wgt * __builtin_amdgcn_sqrtf(v.x * v.x + v.y * v.y);
    };
    // opaque per column: everything derived from the thread index (kept-row indices, near
    // positions, LDS addresses of every pass) is loop-invariant and would otherwise be
    // hoisted out of the column loop into ~90 registers (one workgroup less per CU)
    int tcol = tid;
    asm volatile("" : "+v"(tcol));
    // (what the opaque copy hides and the stored-window tests need: with nstore <= 256, checked by the host, only the
    // first and the last of a thread's 16 rows tid + 256 k3 can lie in the window -- 14 tests fold away)
    __builtin_assume(tcol >= 0 && tcol < MC_WG);
    __builtin_assume(nstore > 0 && nstore <= 256);
    if constexpr (R16) wg_fft4096_r16_tw<+1, 2, 8>(line, tcol, TW, load16, store);
    else wg_fft<H, +1>(line, tcol, tw_col, 1, load, store);
    __syncthreads();  // the next column's first pass overwrites the line
  }
  // rows of the last pass (fft_pass with NS * R == H): y = tid + it * MC_WG + m * (H / R), in
  // the order it-major, m-minor
  if constexpr (R16) {  // wg_fft4096_r16 stores y = tid + 256 k3 in the order k3 = 0..15
#pragma unroll
    for (int k3 = 0; k3 < 16; ++k3) atomicAdd(&bounds[(int64_t)p * H + tid + 256 * k3], acc[k3]);
  } else {
    constexpr int R = (H >= 4096) ? 8 : (H == 2048 ? 4 : 2);  // last radix of FftPlan<H>: 8 8 8 {8,4,2}
    constexpr int NB = H / R, IT = NB / MC_WG;
    static_assert(IT * R == NOUT, "row ownership of the last pass");
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
      for (int m = 0; m < R; ++m)
        atomicAdd(&bounds[(int64_t)p * H + tid + it * MC_WG + m * NB], acc[it * R + m]);
  }
}

// ------------------------------------------------------------------ host dispatch
// mc_xc_col_engine(): 0 = automatic, 1 = always the radix-8 Stockham columns.  Automatic: 1024-point columns
// with at most 128 kept rows at either end go to the wave-per-column kernels, 4096-point columns with at most
// 512 to the register-resident radix-16 ones.
static int g_col_engine = 0;
static bool cols_wave1024(const XcGeom& g) { return g.H == 1024 && g.kyp <= 128 && g.kyn <= 128 && g_col_engine == 0; }
static bool cols_r16(const XcGeom& g) { return g.H == 4096 && g.kyp <= 512 && g.kyn <= 512 && g_col_engine == 0; }

int mc_launch_cols_inv_near(const cfloat* S_cur, const int* cur_idx, const cfloat* S_ref, const int* ref_idx,
                            cfloat* T2n, float* bounds, const cfloat* tw_col, float scale, const XcGeom& g, int nstore,
                            int npairs, hipStream_t stream) {
  auto launch = [&](auto kernel, int cols_per_group) {
    hipLaunchKernelGGL(kernel, dim3((g.nkx + cols_per_group - 1) / cols_per_group, npairs), dim3(256), 0, stream, S_cur,
                       cur_idx, S_ref, ref_idx, T2n, bounds, tw_col, scale, g, nstore);
  };
  static_assert(MC_WG == 256, "one block size for all three");
  if (cols_wave1024(g)) {
    launch(xc_cols_inv_near_wave1024, 4 * XC_NEAR_COLS_W);
  } else if (cols_r16(g)) {
    launch(xc_cols_inv_near<12, true>, XC_NEAR_COLS);
  } else
  MC_DISPATCH_LOG(mc_ilog2(g.H), {
    if constexpr (L >= 10) launch(xc_cols_inv_near<L>, XC_NEAR_COLS);
    else return MC_ERR_UNSUPPORTED;
  });
  return mc_check_launch();
}

// MODE 0, one workgroup per column of the full map
static int cols_inv_full(const cfloat* S_cur, const int* cur_idx, const cfloat* S_ref, const int* ref_idx, cfloat* T2,
                         const cfloat* tw_col, float scale, const XcGeom& g, const int* gate, int npairs,
                         hipStream_t stream) {
  MC_DISPATCH_LOG(mc_ilog2(g.H), {
    hipLaunchKernelGGL((xc_cols_inv<L, 0>), dim3(g.nkx, npairs), dim3(MC_WG), 0, stream, S_cur, cur_idx, S_ref,
                       ref_idx, (const float*)nullptr, T2, tw_col, scale, g, gate);
  });
  return MC_OK;
}
int mc_launch_cols_inv_gated(const cfloat* S_cur, const int* cur_idx, const cfloat* S_ref, const int* ref_idx,
                             cfloat* T2, const cfloat* tw_col, float scale, const XcGeom& g, const int* gate,
                             int npairs, hipStream_t stream) {
  return cols_inv_full(S_cur, cur_idx, S_ref, ref_idx, T2, tw_col, scale, g, gate, npairs, stream);
}

extern "C" {

int mc_xc_col_engine(int mode) {
  if (mode < 0 || mode > 1) return MC_ERR_ARG;
  g_col_engine = mode;
  return MC_OK;
}

int mc_xc_cols_forward(const void* T1, const float* filt, void* S, const void* tw_col, int njobs,
                       const mc_xc_geom* q, void* stream) {
  return mc_xc_cols_forward_fix(T1, filt, S, tw_col, njobs, q, nullptr, nullptr, stream);
}

int mc_xc_cols_forward_fix(const void* T1, const float* filt, void* S, const void* tw_col,
                           int njobs, const mc_xc_geom* q, const float* fix, const void* Mhat,
                           void* stream) {
  XcGeom g;
  int rc = geom_from(q, &g, false, true);
  if (rc) return rc;
  if (!T1 || !S || !tw_col || njobs < 1 || (fix && !Mhat)) return MC_ERR_ARG;
  auto launch = [&](auto kernel, int cols_per_group) {
    hipLaunchKernelGGL(kernel, dim3((g.nkx + cols_per_group - 1) / cols_per_group, njobs), dim3(256), 0,
                       (hipStream_t)stream, (const cfloat*)T1, filt, (cfloat*)S, (const cfloat*)tw_col, g, fix,
                       (const cfloat*)Mhat);
  };
  if (cols_wave1024(g)) launch(xc_cols_fwd_wave1024, 4 * XC_FWDW_COLS);
  else if (cols_r16(g)) launch(xc_cols_fwd<12, true>, XC_FWD_COLS);
  else MC_DISPATCH_LOG(mc_ilog2(g.H), launch(xc_cols_fwd<L>, 1));
  return mc_check_launch();
}

int mc_xc_cols_inverse(const void* S_cur, const int* cur_idx, const void* S_ref,
                       const int* ref_idx, void* T2, const void* tw_col, float scale, int npairs,
                       const mc_xc_geom* q, void* stream) {
  XcGeom g;
  int rc = geom_from(q, &g, false, true);
  if (rc) return rc;
  if (!S_cur || !cur_idx || !S_ref || !ref_idx || !T2 || !tw_col || npairs < 1) return MC_ERR_ARG;
  if (cols_wave1024(g)) {
    hipLaunchKernelGGL(xc_cols_inv_wave1024, dim3((g.nkx + 3) / 4, npairs), dim3(256), 0, (hipStream_t)stream,
                       (const cfloat*)S_cur, cur_idx, (const cfloat*)S_ref, ref_idx, (cfloat*)T2,
                       (const cfloat*)tw_col, scale, g);
    return mc_check_launch();
  }
  rc = cols_inv_full((const cfloat*)S_cur, cur_idx, (const cfloat*)S_ref, ref_idx, (cfloat*)T2, (const cfloat*)tw_col,
                     scale, g, nullptr, npairs, (hipStream_t)stream);
  return rc ? rc : mc_check_launch();
}

int mc_fourier_shift_cols_inverse(const void* S, const int* idx, const float* shifts, void* T2,
                                  const void* tw_col, float scale, int nframes,
                                  const mc_xc_geom* q, void* stream) {
  XcGeom g;
  int rc = geom_from(q, &g, false, true);
  if (rc) return rc;
  if (!S || !idx || !shifts || !T2 || !tw_col || nframes < 1) return MC_ERR_ARG;
  dim3 grid(g.nkx, nframes);
  MC_DISPATCH_LOG(mc_ilog2(g.H), {
    hipLaunchKernelGGL((xc_cols_inv<L, 1>), grid, dim3(MC_WG), 0, (hipStream_t)stream,
                       (const cfloat*)S, idx, (const cfloat*)nullptr, (const int*)nullptr, shifts,
                       (cfloat*)T2, (const cfloat*)tw_col, scale, g, (const int*)nullptr);
  });
  return mc_check_launch();
}

}  // extern "C"
