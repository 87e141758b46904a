"""Greedy mask NMS (reference models/functions/nms.py:53-81) restated in numpy, and the seeded cases the mask-NMS tests share.

Two restatements:
  reference_loop   the reference's double loop, pair by pair: fp32 intersection, fp32 union from the CALLER's sums, fp32 comparison with
                   the threshold rounded to fp32
  row_vectorised   the pairwise decisions as one [n, n] matrix, then `keep[i+1:] &= ~suppress[i, i+1:]` for every kept i (large n)

Cases: `cases()` -> {name: (labels int64 [n], masks bool [n,h,w], sums fp32 [n], thr)} in descending score order -- the hand-made ones
(threshold ties and their one-pixel-over neighbours, a chain, empty masks, doubled sums, the packer's over-read trap) and a seeded family
of rectangles clustered round n/4 centres.  tests/golden/make_golden_mask_nms.py runs the real reference on them and stores its `keep`
vectors in tests/golden/mask_nms.npz; the masks themselves are regenerated from the seeds."""
from collections import OrderedDict

import numpy as np


def reference_loop(labels, masks, sums, thr):
    """-> keep uint8 [n]"""
    n = len(labels)
    if n == 0:
        return np.ones(0, np.uint8)
    flat = np.asarray(masks).reshape(n, -1) != 0
    sums = np.asarray(sums, np.float32)
    t = np.float32(thr)
    keep = np.ones(n, np.uint8)
    for i in range(n - 1):
        if not keep[i]:
            continue
        for j in range(i + 1, n):
            if not keep[j] or labels[i] != labels[j]:
                continue
            inter = np.float32(np.count_nonzero(flat[i] & flat[j]))
            union = np.float32(np.float32(sums[i] + sums[j]) - inter)
            if union > 0:
                if np.float32(inter / union) > t:
                    keep[j] = 0
            else:
                keep[j] = 0
    return keep


def suppress_matrix(labels, masks, sums, thr):
    """[n, n] bool: would i remove j (labels equal, union <= 0 or inter / union > thr in fp32); all pairs, the caller takes i < j"""
    n = len(labels)
    flat = (np.asarray(masks).reshape(n, -1) != 0).astype(np.float32)
    inter = flat @ flat.T                                        # integers < 2^24: exact in fp32 in any summation order
    sums = np.asarray(sums, np.float32)
    union = (sums[:, None] + sums[None, :]) - inter
    labels = np.asarray(labels)
    with np.errstate(divide="ignore", invalid="ignore"):
        over = (inter / union) > np.float32(thr)
    return (labels[:, None] == labels[None, :]) & ((union <= 0) | over)


def row_vectorised(labels, masks, sums, thr):
    """-> keep uint8 [n]"""
    n = len(labels)
    if n == 0:
        return np.ones(0, np.uint8)
    sup = suppress_matrix(labels, masks, sums, thr)
    keep = np.ones(n, bool)
    for i in range(n - 1):
        if keep[i]:
            keep[i + 1:] &= ~sup[i, i + 1:]
    return keep.astype(np.uint8)


def clustered(seed, n, h, w, n_labels=1, drop=0.05):
    """n rectangles round max(1, n // 4) centres with jittered position and size, a few pixels knocked out of each; labels uniform over
    n_labels.  -> (labels int64 [n], masks bool [n,h,w], sums fp32 [n], scores fp32 [n] descending)"""
    rng = np.random.RandomState(seed)
    nc = max(1, n // 4)
    cy, cx = rng.randint(0, h, nc), rng.randint(0, w, nc)
    bh, bw = rng.randint(max(1, h // 8), max(2, h // 3) + 1, nc), rng.randint(max(1, w // 8), max(2, w // 3) + 1, nc)
    masks = np.zeros((n, h, w), bool)
    which = rng.randint(0, nc, n)
    jy, jx = max(1, h // 16), max(1, w // 16)
    for m in range(n):
        c = which[m]
        y0 = cy[c] - bh[c] // 2 + rng.randint(-jy, jy + 1)
        x0 = cx[c] - bw[c] // 2 + rng.randint(-jx, jx + 1)
        y1 = y0 + max(1, bh[c] + rng.randint(-jy, jy + 1))
        x1 = x0 + max(1, bw[c] + rng.randint(-jx, jx + 1))
        masks[m, max(0, y0):max(0, y1), max(0, x0):max(0, x1)] = True
        masks[m] &= rng.rand(h, w) >= drop
    labels = rng.randint(0, n_labels, n).astype(np.int64)
    scores = np.sort(rng.rand(n).astype(np.float32))[::-1].copy()
    return labels, masks, masks.reshape(n, h * w).sum(1).astype(np.float32), scores


def _strip(width, *runs):
    """[len(runs), 1, width] masks; run = (first, last) inclusive pixel range, or None for an empty mask"""
    m = np.zeros((len(runs), 1, width), bool)
    for k, r in enumerate(runs):
        if r is not None:
            m[k, 0, r[0]:r[1] + 1] = True
    return m


def _areas(masks):
    return masks.reshape(len(masks), -1).sum(1).astype(np.float32)


def hand_cases():
    """{name: (labels, masks, sums, thr, expected keep)} -- `expected` is what the arithmetic above gives by hand; the fixture holds what the
    reference gave."""
    z = lambda n: np.zeros(n, np.int64)      # noqa: E731
    out = OrderedDict()

    def add(name, labels, masks, thr, expected, sums=None):
        out[name] = (labels, masks, _areas(masks) if sums is None else np.asarray(sums, np.float32), thr, np.asarray(expected, np.uint8))
    # IoU exactly at the threshold is kept (fp32 quotient against the fp32 threshold; in double 3/10 and 1/3 would be removed) ...
    add("tie_3_of_10", z(2), _strip(20, (0, 6), (4, 9)), 0.3, [1, 1])
    add("tie_1_of_3", z(2), _strip(20, (0, 1), (1, 2)), 1.0 / 3.0, [1, 1])
    add("tie_2_of_4", z(2), _strip(20, (0, 2), (1, 3)), 0.5, [1, 1])
    # ... and a neighbour one pixel over it is removed
    add("over_4_of_10", z(2), _strip(20, (0, 6), (3, 9)), 0.3, [1, 0])
    add("over_2_of_3", z(2), _strip(20, (0, 1), (0, 2)), 1.0 / 3.0, [1, 0])
    add("over_3_of_4", z(2), _strip(20, (0, 2), (0, 3)), 0.5, [1, 0])
    # greedy: B falls to A, so it no longer removes C (A-B 7/13, B-C 7/13, A-C 4/16)
    chain = _strip(20, (0, 9), (3, 12), (6, 15))
    add("chain", z(3), chain, 0.5, [1, 0, 1])
    # the caller's sums are used, not the masks' areas: doubled, A-B is 7/33
    add("chain_sums_doubled", z(3), chain, 0.5, [1, 1, 1], sums=2 * _areas(chain))
    # union <= 0: the later of two empty masks of one label goes; another label and a non-empty mask stay
    add("empty", np.array([0, 0, 1, 0], np.int64), _strip(20, None, None, None, (2, 8)), 0.5, [1, 0, 1, 1])
    # H*W = 33: word 1 of a mask holds ONE pixel.  A packer reading 32 bytes there would take the next mask's first 31 pixels for its
    # own: mask 0 = {32}, masks 1 and 2 = {0..30}.  Rightly 0-1 do not meet and 2 falls to 1
    add("overread_hw33", z(3), _strip(33, (32, 32), (0, 30), (0, 30)), 0.5, [1, 1, 0])
    # bit 31 of a 64-candidate suppression word: candidate 31 repeats candidate 0, everyone else is a pixel of their own
    # (a word handled as two signed halves would smear that bit over candidates 32-63)
    runs = [(k, k) for k in range(40)]
    runs[0] = runs[31] = (50, 59)
    add("bit31_of_a_word", z(40), _strip(64, *runs), 0.5, [int(k != 31) for k in range(40)])
    return out


# (name, seed, n, h, w, labels, thr) of the seeded family in the fixture: n at the 64-bit word edges, up to three labels
RANDOM_CASES = [("rand_n1", 101, 1, 24, 32, 1, 0.5), ("rand_n2", 102, 2, 24, 32, 1, 0.5), ("rand_n63", 103, 63, 24, 32, 1, 0.5),
                ("rand_n64", 104, 64, 24, 32, 2, 0.3), ("rand_n65", 105, 65, 24, 32, 1, 0.3), ("rand_n130_l3", 106, 130, 24, 32, 3, 0.5),
                ("rand_n200", 107, 200, 30, 40, 2, 0.1)]


def cases():
    """{name: (labels, masks, sums, thr)}: the hand-made cases, then the seeded family"""
    out = OrderedDict((k, v[:4]) for k, v in hand_cases().items())
    for name, seed, n, h, w, nl, thr in RANDOM_CASES:
        labels, masks, sums, _ = clustered(seed, n, h, w, nl)
        out[name] = (labels, masks, sums, thr)
    return out
