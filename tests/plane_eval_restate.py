"""Plain-numpy restatement of planerecnet_amd/plane_eval.py, written from the definitions and sharing no code with the
module: a per-pixel loop for the paint, a per-pixel dictionary for the tables, and the dense [A+1, B+1, H, W] broadcast formulation -- the one
PlaneRCNN's evaluateMasks / evaluatePlanesTensor use -- of RI / VOI / SC and the recall curves, in fp64, for small images."""
import numpy as np

SCALE = 2 ** 20


def paint(masks, priority="first"):
    """masks [N,H,W] (non-zero = set) -> int32 [H,W]; per pixel, the first (or last) mask that sets it"""
    masks = np.asarray(masks)
    N, H, W = masks.shape
    out = np.zeros((H, W), np.int32)
    order = range(N) if priority == "first" else range(N - 1, -1, -1)
    for y in range(H):
        for x in range(W):
            for i in order:
                if masks[i, y, x]:
                    out[y, x] = i + 1
                    break
    return out


def paint_fast(masks, priority="first"):
    """the same by argmax, for the large frames"""
    m = np.asarray(masks) != 0
    N = m.shape[0]
    if N == 0:
        return np.zeros(m.shape[1:], np.int32)
    if priority == "first":
        idx = np.argmax(m, 0)
    else:
        idx = N - 1 - np.argmax(m[::-1], 0)
    return np.where(m.any(0), idx + 1, 0).astype(np.int32)


def quantise(depth_a, depth_b):
    """q = rint(fmin(|b - a|, 1024) * 2^20) in fp32, 0 where a < 1e-4 -> python ints via uint64"""
    a, b = np.asarray(depth_a, np.float32), np.asarray(depth_b, np.float32)
    with np.errstate(invalid="ignore"):
        e = np.abs(b - a)
        assert e.dtype == np.float32
        e[a < np.float32(1e-4)] = np.float32(0)
        q = np.rint(np.fmin(e, np.float32(1024)) * np.float32(SCALE))
    assert q.dtype == np.float32
    return q.astype(np.uint64)


def tables(la, lb, na, nb, depth_a=None, depth_b=None):
    """la, lb int [H,W] -> (T, S) int64 [na+1, nb+1], pixel by pixel through a dictionary"""
    la, lb = np.asarray(la), np.asarray(lb)
    q = quantise(depth_a, depth_b) if depth_a is not None else np.zeros(la.shape, np.uint64)
    cells = {}
    for a, b, v in zip(la.reshape(-1).tolist(), lb.reshape(-1).tolist(), q.reshape(-1).tolist()):
        if 0 <= a <= na and 0 <= b <= nb:
            c = cells.setdefault((a, b), [0, 0])
            c[0] += 1
            c[1] += v
    T, S = np.zeros((na + 1, nb + 1), np.int64), np.zeros((na + 1, nb + 1), np.int64)
    for (a, b), (n, s) in cells.items():
        T[a, b], S[a, b] = n, s
    return T, S


def tables_fast(la, lb, na, nb, depth_a=None, depth_b=None):
    """the same by bincount, for the large frames"""
    la, lb = np.asarray(la).reshape(-1).astype(np.int64), np.asarray(lb).reshape(-1).astype(np.int64)
    ok = (la >= 0) & (la <= na) & (lb >= 0) & (lb <= nb)
    idx = la[ok] * (nb + 1) + lb[ok]
    bins = (na + 1) * (nb + 1)
    T = np.bincount(idx, minlength=bins).astype(np.int64).reshape(na + 1, nb + 1)
    S = np.zeros(bins, np.int64)
    if depth_a is not None:
        np.add.at(S, idx, quantise(depth_a, depth_b).reshape(-1)[ok].astype(np.int64))
    return T, S.reshape(na + 1, nb + 1)


# ---- the dense formulation ----------------------------------------------------------------------------------------------------------

def _one_hot(labels, n):
    """[H,W] -> fp64 [n+1,H,W]: plane k's mask in row k, the complement (label 0) in row 0"""
    return (np.asarray(labels)[None] == np.arange(n + 1)[:, None, None]).astype(np.float64)


def dense_scores(la, lb, na, nb):
    """(RI, VOI, SC) as the published protocol computes them: masks broadcast to [na+1, nb+1, H, W] over the pixels the ground truth marks planar,
    the complement of the predicted masks counted as a segment; fp64, no clamp in the logarithms"""
    la, lb = np.asarray(la), np.asarray(lb)
    valid = (la > 0).astype(np.float64)
    gt = _one_hot(la, na)[1:] * valid                                # [na,H,W]
    pred = _one_hot(lb, nb) * valid                                  # [nb+1,H,W]: row 0 = no detection
    N = valid.sum()
    if N < 2:
        return float("nan"), float("nan"), float("nan")
    inter = (gt[:, None] * pred[None]).sum((2, 3))                   # [na, nb+1]
    a, b = gt.sum((1, 2)), pred.sum((1, 2))
    # Rand index by its definition over pixel pairs: pairs together in both, plus pairs apart in both
    pairs = N * (N - 1) / 2
    same_both = (inter * (inter - 1) / 2).sum()
    same_a, same_b = (a * (a - 1) / 2).sum(), (b * (b - 1) / 2).sum()
    ri = (same_both + (pairs - same_a - same_b + same_both)) / pairs
    joint = inter / N
    pa, pb = a / N, b / N
    h = lambda p: -sum(v * np.log2(v) for v in p.reshape(-1).tolist() if v > 0)      # noqa: E731
    mi = sum(joint[g, p] * np.log2(joint[g, p] / (pa[g] * pb[p])) for g in range(joint.shape[0]) for p in range(joint.shape[1]) if joint[g, p] > 0)
    voi = h(pa) + h(pb) - 2 * mi
    union = np.maximum(gt[:, None], pred[None]).sum((2, 3))
    iou = np.where(union > 0, inter / np.where(union > 0, union, 1), 0.0)
    sc = ((a * iou.max(1)).sum() + (b * iou.max(0)).sum()) / (2 * N)
    return float(ri), float(voi), float(sc)


def dense_curves(la, lb, na, nb, depth_a, depth_b, thresholds=None, iou=0.5):
    """(plane recall, pixel recall): masks broadcast to [na, nb, H, W]; the mean depth error of a pair from the quantised per-pixel errors"""
    thresholds = 0.05 * np.arange(21) if thresholds is None else np.asarray(thresholds, np.float64)
    if na == 0:
        return np.full(thresholds.shape, np.nan), np.full(thresholds.shape, np.nan)
    gt, pred = _one_hot(la, na)[1:], _one_hot(lb, nb)[1:]
    err = quantise(depth_a, depth_b).astype(np.float64).reshape(np.asarray(la).shape)
    both = gt[:, None] * pred[None]                                  # [na,nb,H,W]
    inter = both.sum((2, 3))
    a, b = gt.sum((1, 2)), pred.sum((1, 2))
    union = a[:, None] + b[None, :] - inter
    ious = np.where(union > 0, inter / np.where(union > 0, union, 1), 0.0)
    D = np.where(inter > 0, (both * err).sum((2, 3)) / (np.where(inter > 0, inter, 1) * SCALE), 1e6)
    plane, pixel = [], []
    for t in thresholds.tolist():
        match = (ious > iou) & (D <= t)
        plane.append(match.any(1).sum() / float(na))
        pixel.append(np.minimum((inter * match).sum(1), a).sum() / a.sum() if a.sum() > 0 else np.nan)
    return np.asarray(plane), np.asarray(pixel)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------

def random_masks(seed, n, H, W, fill=0.5, dtype=bool):
    """n overlapping rectangles with a few holes; some pixels stay unclaimed"""
    rng = np.random.RandomState(seed)
    out = np.zeros((n, H, W), bool)
    for i in range(n):
        h, w = rng.randint(1, max(2, int(H * fill) + 1)), rng.randint(1, max(2, int(W * fill) + 1))
        y, x = rng.randint(0, H - h + 1), rng.randint(0, W - w + 1)
        out[i, y:y + h, x:x + w] = True
        out[i] &= rng.rand(H, W) > 0.05
    if dtype is bool:
        return out
    return (out * rng.randint(1, 256, out.shape)).astype(np.uint8)


def random_labels(seed, n, H, W, block=4):
    """a label map of blocky segments with labels in [0, n]"""
    rng = np.random.RandomState(seed)
    small = rng.randint(0, n + 1, ((H + block - 1) // block, (W + block - 1) // block))
    return np.kron(small, np.ones((block, block), np.int64))[:H, :W].astype(np.int32)


def random_depths(seed, H, W):
    rng = np.random.RandomState(seed)
    gt = (0.5 + 4.0 * rng.rand(H, W)).astype(np.float32)
    gt[rng.rand(H, W) < 0.1] = 0.0                                   # no ground truth
    pred = (gt + rng.randn(H, W) * 0.3).astype(np.float32)
    return gt, pred
