"""Golden vectors for greedy mask NMS -- runs ONLY in the build container (needs the reference).

    python tests/golden/make_golden_mask_nms.py

Imports the reference's own `mask_nms` (models/functions/nms.py:53-81), runs it on every case of tests/mask_nms_restate.py (hand-made
ties / chain / empty masks / doubled sums / over-read trap, and the seeded clustered-rectangle family) and stores its `keep` vectors in
tests/golden/mask_nms.npz, together with every case's mask areas as a drift check of the seeded generators.  The masks are regenerated from
the seeds by the tests, so the file holds a few KB.  Asserts that the hand-derived expectations hold, that both restatements reproduce
every stored vector, and that in every random case with n >= 63 the reference keeps between 10 % and 90 % (neither everything nor
nothing: the greedy order matters)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_shim  # noqa: E402
import mask_nms_restate as R  # noqa: E402


def main():
    ref_shim.install()
    from models.functions.nms import mask_nms as ref_mask_nms
    hand = R.hand_cases()
    data = {}
    for name, (labels, masks, sums, thr) in R.cases().items():
        n = len(labels)
        scores = torch.linspace(0.9, 0.1, n)                                            # (the reference reads only their length and shape)
        keep = ref_mask_nms(torch.from_numpy(labels), torch.from_numpy(masks), torch.from_numpy(sums), scores, nms_thr=thr)
        keep = keep.numpy().astype(np.uint8)
        if name in hand:
            assert np.array_equal(keep, hand[name][4]), (name, keep, hand[name][4])
        assert np.array_equal(R.reference_loop(labels, masks, sums, thr), keep), name
        assert np.array_equal(R.row_vectorised(labels, masks, sums, thr), keep), name
        frac = float(keep.mean())
        if name.startswith("rand") and n >= 63:
            assert 0.10 <= frac <= 0.90, (name, frac)
        print("%-20s n %3d  kept %3d (%.0f %%)" % (name, n, int(keep.sum()), 100 * frac))
        data["keep_" + name] = keep
        data["area_" + name] = masks.reshape(n, -1).sum(1).astype(np.int32)
    np.savez_compressed(os.path.join(HERE, "mask_nms.npz"), **data)
    print("wrote", os.path.join(HERE, "mask_nms.npz"), os.path.getsize(os.path.join(HERE, "mask_nms.npz")), "bytes")


if __name__ == "__main__":
    main()
