// What more than one of K1's objects uses (xc_common.h has the map of the passes): xc_rows_fwd.hip -- the entry
// points, the route rules, the kernels of the fused frame statistics and of the hot-pixel correction -- and the
// three forward row engines it routes to, xc_rows_fwd_wg.hip, xc_rows_fwd_wave.hip and xc_rows_fwd_wave512.hip.
#pragma once
#include "xc_common.h"

#define XC_STAT_SLOTS 64  // stats_acc = XC_STAT_SLOTS x {sum, sumsq} doubles

// The variant of the wave-per-row kernel a job runs (k1_wave_variant, xc_rows_fwd.hip): one or two kept bins per
// lane and slot (nkx <= 256 or <= 512), and which 256-sample chunks of a row are loaded and how they are clamped
enum K1WaveLoads {
  K1_LOADS_ALL,          // all 16 chunks, each clamped to the support box, or to the row's chord given a table
  K1_LOADS_INNER,        // chunks 1 .. 14; only the first and the last of them clamped, to the support box
  K1_LOADS_INNER_CHORD,  // chunks 1 .. 14, each clamped to the row's chord (with statistics only)
  K1_LOADS_HALF,         // fp16 samples: as K1_LOADS_ALL (with statistics only)
};
struct K1WaveVariant {
  bool keep1;
  K1WaveLoads loads;
};

// A kernel cannot be launched from another object without relocatable device code, so each engine's object
// defines the launcher through which xc_rows_fwd.hip reaches it; none of these is part of the C ABI.  The
// router has checked every argument and the engine's shape and alignment rules.  `raw`: 0 = fp32 (or, wave engine
// with K1_LOADS_HALF, fp16) samples, 1 = u8, 2 = i16 with `gain` and `job_sub`; statistics iff stats_acc != NULL.
// xc_rows_fwd_wg.hip: MC_ERR_ARG when the row lines and the staging tile do not fit a CU's LDS
__attribute__((visibility("hidden"))) int k1_wg_launch(int raw, const void* src, const int64_t* job_off,
                                                       int64_t row_stride, const int* job_expo, const float* mask,
                                                       const float* mean_rstd, void* T1, const void* tw_row, int njobs,
                                                       const XcGeom& g, const XcBox& b, double* stats_acc,
                                                       const float* gain, const float* job_sub, void* stream);
// xc_rows_fwd_wave.hip; raw samples run K1_LOADS_ALL without statistics; MC_ERR_UNSUPPORTED for a statistics-only
// variant without statistics
__attribute__((visibility("hidden"))) int k1_wave_launch(K1WaveVariant v, int raw, const void* src,
                                                         const int64_t* job_off, int64_t row_stride, const float* mask,
                                                         const float* mean_rstd, void* T1, const void* tw_row,
                                                         int njobs, const XcGeom& g, const XcBox& b, double* stats_acc,
                                                         const int* row_chord, const float* gain, const float* job_sub,
                                                         void* stream);
// xc_rows_fwd_wave512.hip: samples of any `storage` (MC_STORE_*); two spectra per job iff expo_b != NULL
__attribute__((visibility("hidden"))) int k1_wave512_launch(int storage, const void* src, const int64_t* job_off,
                                                            int64_t row_stride, const int* expo_a, const int* expo_b,
                                                            const float* mask, const float* mean_rstd, void* T1a,
                                                            void* T1b, const void* tw_row, int njobs, const XcGeom& g,
                                                            const int* row_chord, const float* gain, int64_t frame_area,
                                                            const float* job_sub, void* stream);
