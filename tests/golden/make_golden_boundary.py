"""Writes tests/golden/boundary_cases.npz: a few masks of tests/morphology_restate.py at two sizes with scipy.ndimage's answers --
binary_erosion / binary_dilation with the 3 x 3 all-ones element, iterations = r, border_value 0 and 1; the inner bands
m & ~binary_erosion(m, ..., border_value=0); and the fp32 mask IoU and boundary IoU matrices of the first `split` masks against the rest.
The tests then need no scipy.  Masks are stored bit-packed, everything compressed.

    python tests/golden/make_golden_boundary.py
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import morphology_restate as R      # noqa: E402

FULL = np.ones((3, 3), bool)
# tag: (H, W), radii -- one word and a bit per row with radii inside a word, across a word and beyond the image; two words and a bit, the metric-sized radius
CASES = {"a": ((37, 65), (1, 3, 33, 70)), "b": ((66, 130), (2, 16))}
NAMES = ("blob0", "blob1", "blob2", "checker", "frame", "full", "hole_c", "rect3_sq")


def scipy_erode(m, r, border):
    return np.stack([ndimage.binary_erosion(x, FULL, iterations=r, border_value=border) for x in m])


def scipy_dilate(m, r, border):
    return np.stack([ndimage.binary_dilation(x, FULL, iterations=r, border_value=border) for x in m])


def iou_f32(a, b):
    out = np.zeros((len(a), len(b)), np.float32)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            inter = np.float32((x & y).sum())
            with np.errstate(invalid="ignore", divide="ignore"):
                out[i, j] = inter / ((np.float32(x.sum()) + np.float32(y.sum())) - inter)
    return out


def main():
    out = {}
    for tag, ((H, W), radii) in CASES.items():
        P = R.patterns(H, W)
        masks = np.stack([np.zeros((H, W), bool)] + [P[k] for k in NAMES] + [np.zeros((H, W), bool)])      # (an empty mask on either side: one 0/0)
        split = 4
        out["names_" + tag] = np.array(("empty",) + NAMES + ("empty",))
        out["shape_" + tag] = np.array(masks.shape, np.int32)
        out["radii_" + tag] = np.array(radii, np.int32)
        out["split_" + tag] = np.int32(split)
        out["masks_" + tag] = np.packbits(masks)
        for r in radii:
            for b in (0, 1):
                out["erode_%s_r%d_b%d" % (tag, r, b)] = np.packbits(scipy_erode(masks, r, b))
                out["dilate_%s_r%d_b%d" % (tag, r, b)] = np.packbits(scipy_dilate(masks, r, b))
            band = masks & ~scipy_erode(masks, r, 0)
            out["band_%s_r%d" % (tag, r)] = np.packbits(band)
            out["miou_%s_r%d" % (tag, r)] = iou_f32(masks[:split], masks[split:])
            out["biou_%s_r%d" % (tag, r)] = iou_f32(band[:split], band[split:])
    path = os.path.join(HERE, "boundary_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
