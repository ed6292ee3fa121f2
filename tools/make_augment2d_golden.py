"""Record what PIL computes for the 2-D rotation contract of hdf_augment_2d (include/hdf.h) into
tests/golden/augment2d_pil.npz: per (shape, angle) case the inputs of tests/augment2d_ref.py and
Image.fromarray(channel).rotate(angle, Image.BILINEAR) per fp32 channel, Image.fromarray(labels).rotate(angle,
Image.NEAREST) for the uint8 class map -- the two calls of RandomRotate2D (data_utils/transformer_2d.py:161-169).
tests/test_augment2d_ref_cpu.py holds the numpy restatement to this file bit for bit, with or without PIL installed.

    python tools/make_augment2d_golden.py            # needs PIL; rewrites the fixture and prints its PIL version"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment2d_ref as ar  # noqa: E402

# (H, W, angle): every shape of the CPU test, the reference's angles, the angles PIL short-cuts (0, 180, square 90) and
# two it does not (non-square 270, 37.3, 181)
CASES = ((24, 24, 10), (24, 24, 90), (24, 24, 0), (17, 29, -5), (17, 29, 270), (40, 33, 15), (40, 33, 181),
         (37, 43, -15), (37, 43, 37.3), (37, 43, 180), (1, 9, 5), (9, 1, -10), (2, 2, 90))
OUT = os.path.join(ROOT, "tests", "golden", "augment2d_pil.npz")


def main():
    import PIL
    from PIL import Image
    arrays = {"cases": np.array(CASES, dtype=np.float64), "pil_version": np.array(PIL.__version__)}
    for k, (h, w, angle) in enumerate(CASES):
        # one channel per image scale of the contract
        image = np.concatenate([ar.image_of((h, w), 1, 10 + k, s) for s in ar.SCALES])
        labels = ar.labels_of((h, w), 10 + k)
        arrays["image_%d" % k] = image
        arrays["labels_%d" % k] = labels
        arrays["pil_image_%d" % k] = np.stack([np.array(Image.fromarray(ch).rotate(angle, Image.BILINEAR))
                                               for ch in image]).astype(np.float32)
        arrays["pil_labels_%d" % k] = np.array(Image.fromarray(labels).rotate(angle, Image.NEAREST)).astype(np.uint8)
    np.savez_compressed(OUT, **arrays)
    print("wrote %s: %d cases, %d bytes, PIL %s" % (OUT, len(CASES), os.path.getsize(OUT), PIL.__version__))


if __name__ == "__main__":
    main()
