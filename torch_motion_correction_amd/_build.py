"""Build libmcorr.so (hand-written HIP kernels + C ABI) for gfx950, in-tree.

``python -m torch_motion_correction_amd._build`` or ``build_library()``.
hipcc cross-compiles without a GPU; the .so is git-ignored but travels with the
source tree to the GPU box.
"""

from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
INCLUDE = os.path.join(os.path.dirname(PKG_DIR), "include")
LIB_PATH = os.path.join(PKG_DIR, "libmcorr.so")
# (source, object stem, extra flags), slowest first.  The generic-length engine is four sources over xcg_common.h,
# one kernel family each: its 101 kernels took five minutes as one translation unit, 75 s each side by side
SOURCES = [("xcg_rows_inv.hip", "xcg_rows_inv", []), ("xcg_cols_inv.hip", "xcg_cols_inv", []),
           ("xcg_rows_fwd.hip", "xcg_rows_fwd", []), ("xcg_cols_fwd.hip", "xcg_cols_fwd", []),
           # the power-of-two engine, one object per pass family (K2-K3 / K4-K6); K1 is four objects over xc_rows_fwd.h:
           # the workgroup and the wave engine here (12 s and 11 s), the patch-row engine and the entry points (3 s and
           # 2 s) further down
           ("xc_rows_fwd_wg.hip", "xc_rows_fwd_wg", []), ("xc_rows_fwd_wave.hip", "xc_rows_fwd_wave", []),
           # row-major full spectra over full_common.h: per-frame transforms / fused sums and the raw row pass
           ("full_fft.hip", "full_fft", []), ("full_sums.hip", "full_sums", []), ("fourier_crop.hip", "fourier_crop", []),
           ("fourier_crop_to.hip", "fourier_crop_to", []),
           ("xc_cols.hip", "xc_cols", []), ("xc_search.hip", "xc_search", []),
           # warp_*.hip and field_tables.hip (one object per kernel family; the field warp is three objects over
           # warp_field_common.h: production kernels, the two fallback kernels, lattice tables and splines): the SLP
           # vectoriser turns the per-pixel coordinate chain into v_pk_* instructions fed by ~1300 v_mov_b32 per
           # kernel and 90 more VGPRs (warp_field 215 -> 160); packed fp32 issues at half the scalar rate on gfx950,
           # so nothing is gained for it
           ("warp_field.hip", "warp_field", ["-fno-slp-vectorize"]),
           ("warp_field_fallback.hip", "warp_field_fallback", ["-fno-slp-vectorize"]),
           ("warp_rigid.hip", "warp_rigid", ["-fno-slp-vectorize"]), ("warp_rigid_raw.hip", "warp_rigid_raw", ["-fno-slp-vectorize"]),
           ("field_tables.hip", "field_tables", ["-fno-slp-vectorize"]),
           # conditioning, statistics and hot pixels of raw movies over cond_common.h; the plan's tables
           ("hot_pixels.hip", "hot_pixels", []), ("condition.hip", "condition", []),
           ("xc_rows_fwd_wave512.hip", "xc_rows_fwd_wave512", []), ("xc_rows_fwd.hip", "xc_rows_fwd", []),
           ("field_post.hip", "field_post", []), ("local_motion.hip", "local_motion", []),
           ("polyphase.hip", "polyphase", []), ("plan_tables.hip", "plan_tables", []), ("xc_refine.hip", "xc_refine", []),
           ("xc_refine_patches.hip", "xc_refine_patches", []), ("raw_accumulate.hip", "raw_accumulate", []),
           ("raw_group.hip", "raw_group", []), ("defect_fill.hip", "defect_fill", []),
           # MRC sample rows -> raw movies, over mrc.h; quarter turns and flips of raw images (the gain)
           ("mrc_decode.hip", "mrc_decode", []), ("raw_orient.hip", "raw_orient", []),
           # raw movies -> MRC sample rows and the header's statistics, over mrc_encode.h
           ("mrc_encode.hip", "mrc_encode", []),
           # EER event movies -> raw u8 movies, over eer.h
           ("eer_render.hip", "eer_render", []),
           # frames through a 2 x 2 linear map, bicubic (magnification distortion), over affine_resample.h
           ("affine_resample.hip", "affine_resample", []),
           # the aligned sum with that map folded into the rigid warp, over affine_warp_sum.h
           ("affine_warp_sum.hip", "affine_warp_sum", []),
           # raw movies -> LZW TIFF strips, over tiff_lzw_encode.h; LZW / stored TIFF strips -> raw movies, over
           # tiff_lzw.h
           ("tiff_encode.hip", "tiff_encode", []), ("tiff_decode.hip", "tiff_decode", [])]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value"]


def _stale(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    mt = os.path.getmtime(target)
    return any(os.path.getmtime(d) > mt for d in deps)


def build_library(force: bool = False, verbose: bool = False) -> str:
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(INCLUDE, "mcorr.h"))
    objdir = os.path.join(PKG_DIR, "build")
    os.makedirs(objdir, exist_ok=True)

    def compile_one(item) -> str:
        src, stem, extra = item
        obj = os.path.join(objdir, stem + ".o")
        srcp = os.path.join(CSRC, src)
        if force or _stale(obj, [srcp] + headers):
            cmd = [HIPCC, *FLAGS, *extra, f"-I{INCLUDE}", f"-I{CSRC}", "-c", srcp, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    if force or _stale(LIB_PATH, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB_PATH]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return LIB_PATH


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
