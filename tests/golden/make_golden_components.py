"""Writes tests/golden/components_cases.npz: the hand-made masks of tests/components_restate.py::patterns at two sizes with
scipy.ndimage's answers -- ndimage.label (full 3x3 structure for connectivity 8, the cross for 4), and for every entry of CLEAN_VARIANTS
the selection by area (bincount; the first maximum on a tie) followed by ndimage.binary_fill_holes with the dual structure.  The tests then
need no scipy.  Masks are stored bit-packed, labels as uint16, everything compressed.

    python tests/golden/make_golden_components.py
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import components_restate as R      # noqa: E402

SIZES = {"a": ((37, 65), (0.1, 0.5, 0.59, 0.9)), "b": ((66, 130), ())}      # (H, W), random densities: one and four 32 x 64 tiles (plus remainders)
CROSS, FULL = ndimage.generate_binary_structure(2, 1), np.ones((3, 3), bool)


def scipy_clean(mask, connectivity, keep, min_area, fill_holes):
    lab, K = ndimage.label(mask, structure=FULL if connectivity == 8 else CROSS)
    areas = np.bincount(lab.ravel(), minlength=K + 1)[1:]
    if keep == "largest":
        chosen = [int(np.argmax(areas)) + 1] if K and areas.max() >= min_area else []
    else:
        chosen = (np.flatnonzero(areas >= min_area) + 1).tolist()
    sel = np.isin(lab, chosen)
    if fill_holes:
        sel = ndimage.binary_fill_holes(sel, structure=CROSS if connectivity == 8 else FULL)
    return sel, (K, len(chosen), int(areas.max()) if K else 0, int(sel.sum()))


def main():
    out = {}
    for tag, ((H, W), dens) in SIZES.items():
        P = R.patterns(H, W, densities=dens)
        names = sorted(P)
        masks = np.stack([P[k] for k in names])
        out["names_" + tag] = np.array(names)
        out["shape_" + tag] = np.array([len(names), H, W], np.int32)
        out["masks_" + tag] = np.packbits(masks)
        for conn in (4, 8):
            labs = [ndimage.label(m, structure=FULL if conn == 8 else CROSS) for m in masks]
            assert max(k for _, k in labs) < 65536
            out["labels%d_%s" % (conn, tag)] = np.stack([lab for lab, _ in labs]).astype(np.uint16)
            out["count%d_%s" % (conn, tag)] = np.array([k for _, k in labs], np.int32)
            for v, (keep, min_area, fill) in enumerate(R.CLEAN_VARIANTS):
                res = [scipy_clean(m, conn, keep, min_area, fill) for m in masks]
                out["clean%d_v%d_%s" % (conn, v, tag)] = np.packbits(np.stack([s for s, _ in res]))
                out["info%d_v%d_%s" % (conn, v, tag)] = np.array([i for _, i in res], np.int32).T.copy()      # rows: count, kept, largest, area
    path = os.path.join(HERE, "components_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
