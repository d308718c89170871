"""Write tests/golden/tiff_lzw_libtiff.npz: small TIFF files written by Pillow's libtiff encoder, and the pixel
arrays they were made from.  They pin the LZW rule of csrc/tiff_lzw.h and tests/tiff_reference.py to an independent
encoder.  Needs Pillow with libtiff; run on a build machine only -- no test imports Pillow.

  python scripts/make_tiff_goldens.py
"""

import io
import os

import numpy as np
from PIL import Image, TiffImagePlugin, features

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                   "tiff_lzw_libtiff.npz")


def tiff_bytes(frames, compression, strip_bytes):
    """the frames as one multi-page TIFF in strips of about `strip_bytes`"""
    TiffImagePlugin.STRIP_SIZE = strip_bytes
    images = [Image.fromarray(f) for f in frames]
    buf = io.BytesIO()
    images[0].save(buf, format="TIFF", save_all=True, append_images=images[1:], compression=compression)
    return np.frombuffer(buf.getvalue(), dtype=np.uint8)


def main():
    assert features.check("libtiff"), "Pillow without libtiff writes no LZW"
    rng = np.random.default_rng(20240519)
    movies = {
        # three frames in strips of 11 rows: RowsPerStrip does not divide h, w is no multiple of 4
        "u8_strips": (rng.poisson(1.0, (3, 70, 100)).astype(np.uint8), "tiff_lzw", 1100),
        # one strip of 60 000 samples: more than 4100 codes, so Clear and all four widths occur inside it
        "u8_long_strip": (rng.poisson(1.0, (1, 100, 600)).astype(np.uint8), "tiff_lzw", 65536),
        "u16": (rng.poisson(300.0, (2, 33, 50)).astype(np.uint16), "tiff_lzw", 1000),
        "f32": ((1.0 + 0.05 * rng.standard_normal((1, 40, 36))).astype(np.float32), "tiff_lzw", 2000),
        "u8_stored": (rng.poisson(2.0, (2, 37, 129)).astype(np.uint8), None, 129 * 5),
    }
    arrays = {}
    for name, (pixels, compression, strip_bytes) in movies.items():
        arrays["file_" + name] = tiff_bytes(pixels, compression, strip_bytes)
        arrays["pixels_" + name] = pixels
    np.savez(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
