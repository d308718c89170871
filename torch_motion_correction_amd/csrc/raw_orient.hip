// Quarter-turn rotations and flips of raw images and movies: numpy.rot90(x, k, axes=(-2, -1)) followed by a flip of
// the rows' order ("ud") or of every row ("lr"), for elements of 1, 2 or 4 bytes.  The gain reference of one program
// oriented for the movie of another; exact, it moves elements.
//
// Every (k, flip) is one of eight maps  out[i][j] = in[y][x]:
//   even k   y = i or h - 1 - i,  x = j or w - 1 - j          orient_rows<E, RX>       a row copy
//   odd k    y = j or h - 1 - j,  x = i or w - 1 - i          orient_transpose<E>      a tiled transpose through LDS
// so the flip costs nothing: it toggles one of the two reversals (ry, rx) on the host.
//
// orient_rows: a thread moves 16 bytes of an output row, 16 / E elements, reversed within the unit when rx; rows
// shorter than a unit, and the last partial unit, go element by element.
//
// orient_transpose: a tile is 128 bytes x 128 bytes on both sides -- 128 / E rows of 128 / E elements, 32 x 32 fp32,
// 64 x 64 int16 / fp16, 128 x 128 uint8 -- so that 8 lanes x 16 bytes read one 128-byte line of an input row and
// 8 lanes x 16 bytes write one of an output row, whatever E.  In LDS a tile row is 32 words + 1 word of padding, and
// every 32 rows are followed by 2 more words: word(r, d) = 33 r + 2 (r / 32) + d.
//   write, row-wise (ds_write_b32 x 4): a 32-lane half holds 4 consecutive rows r x 8 units c, bank = (r + 4 c + q +
//     const) mod 32 for word q of the unit: 32 different banks.
//   read, column-wise (ds_read_b32, the element shifted out of its word): lane (out row ox, unit c) reads rows
//     (16 / E) c + k of word column ox E / 4.  A half holds 4 consecutive ox x 8 c.  E = 4: bank = (4 c + k + ox) mod
//     32, all different.  E = 2: rows 8 c + k, two word columns d, each read by two lanes at one address (a
//     broadcast): bank = (8 c + 2 (c / 4) + k + d) mod 32, all 16 different -- the 2 words after row 31 are what
//     separates c from c + 4.  E = 1: rows 16 c + k, one word column: bank = (16 c + 2 (c / 2) + k) mod 32, all 8
//     different.
// Neither side is bank-conflicted by this count (MI355X: 32 banks for ds_write and ds_read_b32, conflicts counted per
// 32-lane half); it has not been read off a counter.  The reversals are folded into the tile's destination: rx
// mirrors the output row, ry mirrors the output column and the order in which a lane gathers its elements.
#include "mc_common.h"
#include "mcorr.h"

namespace {

constexpr int WG = 256;

struct U16 {
  uint32_t v[4];
};

__device__ __forceinline__ U16 load16(const unsigned char* p) {  // any alignment
  U16 u;
  __builtin_memcpy(&u, p, 16);
  return u;
}
__device__ __forceinline__ void store16(unsigned char* p, const U16& u) { __builtin_memcpy(p, &u, 16); }

template <int E>
__device__ __forceinline__ void copy_element(const unsigned char* src, unsigned char* dst) {
#pragma unroll
  for (int b = 0; b < E; ++b) dst[b] = src[b];
}

// the 16 / E elements of a unit in reverse order
template <int E>
__device__ __forceinline__ U16 reversed(const U16& a) {
  U16 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t x = a.v[3 - k];
    r.v[k] = E == 4 ? x : E == 2 ? (x >> 16) | (x << 16) : __builtin_bswap32(x);
  }
  return r;
}

template <int E, bool RX>
__global__ __launch_bounds__(WG) void orient_rows(const unsigned char* __restrict__ in, int n, int h, int w, int ry,
                                                  unsigned char* __restrict__ out) {
  constexpr int PER = 16 / E;
  const long long j0 = ((long long)blockIdx.x * WG + threadIdx.x) * PER;
  if (j0 >= w) return;
  const long long row = (long long)w * E;
  for (int f = blockIdx.z; f < n; f += gridDim.z)
    for (int i = blockIdx.y; i < h; i += gridDim.y) {
      const unsigned char* src = in + ((long long)f * h + (ry ? h - 1 - i : i)) * row;
      unsigned char* dst = out + ((long long)f * h + i) * row;
      if (j0 + PER <= w) {
        const U16 v = load16(src + (RX ? w - j0 - PER : j0) * E);
        store16(dst + j0 * E, RX ? reversed<E>(v) : v);
      } else {
        for (long long j = j0; j < w; ++j) copy_element<E>(src + (RX ? w - 1 - j : j) * E, dst + j * E);
      }
    }
}

template <int E>
__global__ __launch_bounds__(WG) void orient_transpose(const unsigned char* __restrict__ in, int n, int h, int w,
                                                       int ry, int rx, unsigned char* __restrict__ out) {
  constexpr int T = 128 / E, PER = 16 / E, PASSES = T / 32;
  __shared__ uint32_t tile[T * 33 + (T / 32) * 2];
  const int c = threadIdx.x % 8, rr = threadIdx.x / 8;
  const long long x0 = (long long)blockIdx.x * T;
  const int tiles_y = (h + T - 1) / T;
  for (int f = blockIdx.z; f < n; f += gridDim.z)
    for (int ty = blockIdx.y; ty < tiles_y; ty += gridDim.y) {
      const long long y0 = (long long)ty * T;
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int r = p * 32 + rr;
        const long long y = y0 + r, x = x0 + c * PER;
        U16 v = {{0u, 0u, 0u, 0u}};
        if (y < h && x < w) {
          const unsigned char* src = in + (((long long)f * h + y) * w + x) * E;
          if (x + PER <= w) {
            v = load16(src);
          } else {
            const int left = (int)(w - x) * E;
#pragma unroll
            for (int b = 0; b < 16; ++b)
              if (b < left) v.v[b / 4] |= (uint32_t)src[b] << (8 * (b % 4));
          }
        }
        uint32_t* t = tile + r * 33 + (r / 32) * 2 + c * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = v.v[q];
      }
      __syncthreads();
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int ox = p * 32 + rr;
        const long long x = x0 + ox;
        if (x < w) {
          U16 v = {{0u, 0u, 0u, 0u}};
#pragma unroll
          for (int k = 0; k < PER; ++k) {
            const int r = c * PER + (ry ? PER - 1 - k : k);
            const uint32_t word = tile[r * 33 + (r / 32) * 2 + (ox * E) / 4];
            const uint32_t e = E == 4 ? word : (word >> (8 * ((ox * E) % 4))) & (E == 2 ? 0xffffu : 0xffu);
            v.v[(k * E) / 4] |= e << (8 * ((k * E) % 4));
          }
          const long long j0 = ry ? h - (y0 + c * PER + PER) : y0 + c * PER;  // the output column of element 0
          unsigned char* dst = out + ((long long)f * w + (rx ? w - 1 - x : x)) * h * E;
          if (j0 >= 0 && j0 + PER <= h) {
            store16(dst + j0 * E, v);
          } else {
#pragma unroll
            for (int k = 0; k < PER; ++k) {
              const long long j = j0 + k;
              if (j < 0 || j >= h) continue;
              const uint32_t e = v.v[(k * E) / 4] >> (8 * ((k * E) % 4));
#pragma unroll
              for (int b = 0; b < E; ++b) dst[j * E + b] = (unsigned char)(e >> (8 * b));
            }
          }
        }
      }
      __syncthreads();
    }
}

template <int E>
void launch(const unsigned char* in, int n, int h, int w, bool transpose, int ry, int rx, unsigned char* out,
            hipStream_t st) {
  const unsigned gz = (unsigned)(n < 65535 ? n : 65535);
  if (transpose) {
    constexpr int T = 128 / E;
    const int tiles_y = (h + T - 1) / T;
    const dim3 grid((unsigned)((w + T - 1) / T), (unsigned)(tiles_y < 65535 ? tiles_y : 65535), gz);
    hipLaunchKernelGGL(orient_transpose<E>, grid, dim3(WG), 0, st, in, n, h, w, ry, rx, out);
  } else {
    const long long units = ((long long)w * E + 15) / 16;
    const dim3 grid((unsigned)((units + WG - 1) / WG), (unsigned)(h < 65535 ? h : 65535), gz);
    if (rx) hipLaunchKernelGGL((orient_rows<E, true>), grid, dim3(WG), 0, st, in, n, h, w, ry, out);
    else hipLaunchKernelGGL((orient_rows<E, false>), grid, dim3(WG), 0, st, in, n, h, w, ry, out);
  }
}

}  // namespace

extern "C" int mc_raw_orient(const void* in, int elem_bytes, int n, int h, int w, int rot90, int flip, void* out,
                             void* stream) {
  if (!in || !out || in == out) return MC_ERR_ARG;
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return MC_ERR_ARG;
  if (n < 1 || h < 1 || w < 1 || rot90 < 0 || rot90 > 3 || flip < 0 || flip > 2) return MC_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(in) % elem_bytes || reinterpret_cast<uintptr_t>(out) % elem_bytes)
    return MC_ERR_ARG;
  if ((long long)h * w >= (1ll << 31)) return MC_ERR_UNSUPPORTED;
  // out[i][j] = in[y][x]: rot90 1 is in[j][w - 1 - i], 2 is in[h - 1 - i][w - 1 - j], 3 is in[h - 1 - j][i]
  const bool transpose = rot90 & 1;
  int ry = rot90 >= 2, rx = rot90 == 1 || rot90 == 2;
  // "ud" mirrors i, "lr" mirrors j; under a transpose i indexes x and j indexes y
  if (flip == 1) (transpose ? rx : ry) ^= 1;
  if (flip == 2) (transpose ? ry : rx) ^= 1;
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* i8 = static_cast<const unsigned char*>(in);
  unsigned char* o8 = static_cast<unsigned char*>(out);
  if (elem_bytes == 1) launch<1>(i8, n, h, w, transpose, ry, rx, o8, st);
  else if (elem_bytes == 2) launch<2>(i8, n, h, w, transpose, ry, rx, o8, st);
  else launch<4>(i8, n, h, w, transpose, ry, rx, o8, st);
  return mc_check_launch();
}
