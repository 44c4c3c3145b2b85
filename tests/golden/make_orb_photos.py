"""tests/golden/orb_photos_640.npz, orb_photos_800.npz, orb_photos_1600.npz: the pictures of SiftGPU's own test data
(external/SiftGPU/data) that sift_photo_pairs.npz does not hold, decoded to 8-bit luminance with PIL here and stored,
because neither the reference tree nor a JPEG decoder is assumed at test time:
  640-3, 640-4, 640-5 (640x480), 800-3, 800-4 (800x600), and the central 1024x768 quarter of 1600.jpg (2048x1536), which
  load_photos() in tests/test_oracle_orb_photos.py mirrors into a seamless 2048x1536 image (the whole picture would not
  fit the repository's size limit for one file).
Storage is lossless and needs only numpy and the standard library: the second difference r = x[y,x] - x[y,x-1] -
x[y-1,x] + x[y-1,x-1] (mod 256) of each picture, xz-compressed, as a uint8 array "xz_<name>", next to "shape_<name>" and
the CRC32 of the decoded luminance bytes "crc_<name>".  640-1, 640-2, 800-1 and 800-2 are in sift_photo_pairs.npz.
    python tests/golden/make_orb_photos.py        (needs /root/reference)"""
import lzma
import os
import zlib

import numpy as np
from PIL import Image

DATA = "/root/reference/external/SiftGPU/data"
FILES = {"orb_photos_640.npz": ("640-3", "640-4", "640-5"), "orb_photos_800.npz": ("800-3", "800-4"),
         "orb_photos_1600.npz": ("1600",)}
HERE = os.path.dirname(os.path.abspath(__file__))


def encode(g):
    r = np.diff(np.diff(g.astype(np.int16), axis=1, prepend=0), axis=0, prepend=0).astype(np.uint8)
    return np.frombuffer(lzma.compress(r.tobytes(), preset=9 | lzma.PRESET_EXTREME), np.uint8)


def decode(xz, shape):
    r = np.frombuffer(lzma.decompress(xz.tobytes()), np.uint8).reshape(tuple(int(s) for s in shape))
    return np.ascontiguousarray(np.cumsum(np.cumsum(r, axis=0, dtype=np.uint8), axis=1, dtype=np.uint8))


if __name__ == "__main__":
    for fname, names in FILES.items():
        out = {}
        for name in names:
            g = np.asarray(Image.open(os.path.join(DATA, name + ".jpg")).convert("L"), np.uint8)
            if name == "1600":
                name = "1600q"
                g = g[384:1152, 512:1536]
            g = np.ascontiguousarray(g)
            key = name.replace("-", "_")
            out["xz_" + key] = encode(g)
            out["shape_" + key] = np.array(g.shape, np.int64)
            out["crc_" + key] = np.array(zlib.crc32(g.tobytes()), np.uint32)
            assert np.array_equal(decode(out["xz_" + key], g.shape), g)
            print(name, g.shape, "%08x" % zlib.crc32(g.tobytes()))
        dst = os.path.join(HERE, fname)
        np.savez(dst, **out)
        print(dst, os.path.getsize(dst))
