"""Record what PIL computes for the 2-D zoom contract of hdf_zoom_2d (include/hdf.h) into tests/golden/zoom2d_pil.npz:
per (shape, factor, draws) case of tests/zoom2d_ref.py the two calls of RandomZoom2D (data_utils/transformer_2d.py:
230-264) made for real -- Image.crop or ImageOps.expand, then resize((W, H), BILINEAR) of each mode-F plane (image scales
1 and 1000) and resize((W, H), NEAREST) of the mode-L class map.  The inputs are regenerated from their seeds
(tests/augment2d_ref.py), so the fixture holds the canvas and PIL's results only: a SHA-256 of the result's bytes for
every case, and the arrays themselves for the 24x24 cases, where a mismatch can then be located.
tests/test_zoom2d_ref_cpu.py holds the numpy restatement to this file bit for bit, with or without PIL installed.

    python tools/make_zoom2d_golden.py               # needs PIL; rewrites the fixture and prints its PIL version"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import zoom2d_ref as zr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "zoom2d_pil.npz")
FULL_SHAPE = (24, 24)


def case_inputs(k, shape):
    """the planes of case k: fp32 [len(SCALES), H, W] and uint8 [H, W] with a new byte at nearly every pixel"""
    image = np.concatenate([zr.image_of(shape, 1, 40 + k, s) for s in zr.SCALES])
    return image, zr.labels_of(shape, 40 + k, blocky=False)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    import PIL
    cases, canvases, sha_image, sha_labels, arrays = [], [], [], [], {}
    for shape in zr.SHAPES:
        for factor in zr.FACTORS:
            for draws in zr.zoom_cases(shape, factor):
                k = len(cases)
                image, labels = case_inputs(k, shape)
                planes = [zr.pil_zoom(ch, factor, *draws) for ch in image]
                lab, canvas = zr.pil_zoom(labels, factor, *draws)
                assert all(c == canvas for _, c in planes)
                pil_image = np.stack([p for p, _ in planes])
                cases.append(shape + (factor,) + draws)
                canvases.append(canvas)
                sha_image.append(digest(pil_image))
                sha_labels.append(digest(lab))
                if shape == FULL_SHAPE:
                    arrays["pil_image_%d" % k], arrays["pil_labels_%d" % k] = pil_image, lab
    np.savez_compressed(OUT, cases=np.array(cases, dtype=np.float64), canvases=np.array(canvases, dtype=np.int32),
                        sha_image=np.array(sha_image), sha_labels=np.array(sha_labels),
                        pil_version=np.array(PIL.__version__), **arrays)
    print("wrote %s: %d cases, %d bytes, PIL %s" % (OUT, len(cases), os.path.getsize(OUT), PIL.__version__))


if __name__ == "__main__":
    main()
