"""Plane-level evaluation: the segmentation scores RI / VOI / SC and plane / pixel recall over depth-error thresholds, the figures PlaneNet,
PlaneAE, PlaneRCNN and PlaneRecNet publish (include/prn.h: prn_label_map, prn_label_overlap).

Every one of them is a function of two small integer tables per frame:

  T[g][p]   pixels that carry ground-truth label g and predicted label p (label 0: no mask)
  S[g][p]   the sum over the same pixels of the depth error |pred - gt|, as a fixed-point integer: 0 where gt < 1e-4 (no ground truth),
            else q = rint(fmin(e, 1024) * 2^20), e in fp32 -- NaN and anything above 1024 m count as 1024 m

  label_map   paints [N,H,W] masks into an int32 [H,W] map: 0 = no mask, i + 1 = instance i; where masks overlap, priority "first" gives
              the lowest index (the highest score: detections come sorted by score), "last" the highest (the order planes.planar_depth paints in)
  overlap     (T, S) of two label maps, as int64

Device tensors run on the device (one launch each, integer atomics only, no host synchronisation, inputs untouched; a single tensor is
painted without any upload, a list through a pointer table), CPU tensors on the host in numpy, with the same outputs bit for bit -- the
rule of morphology.erode.  All floating-point scoring happens in fp64 on the host, from
the integers: `segmentation_scores`, `recall_curves`.  `PlaneEvalAccumulator` does a whole evaluation run: two paints and one table
call per frame, the tables stay on the device and come down once at the end.
"""
import numpy as np
import torch

from ._masks import _as_bytes, _describe, _inputs, _p, _stream, _upload

__all__ = ["label_map", "overlap", "segmentation_scores", "recall_curves", "PlaneEvalAccumulator", "LDS_BINS", "MAX_LABEL", "DEPTH_SCALE", "DEPTH_CAP",
           "THRESHOLDS"]

LDS_BINS = 4096                    # up to this (na + 1) * (nb + 1) a workgroup keeps its tables in LDS (include/prn.h: PRN_LABEL_OVERLAP_LDS_BINS)
MAX_LABEL = 1023                   # the largest na / nb
DEPTH_SCALE = 1 << 20              # fixed-point units per metre
DEPTH_CAP = 1024.0                 # metres: the largest error a pixel contributes
THRESHOLDS = 0.05 * np.arange(21)  # metres: the depth-error thresholds of the recall curves (0 .. 1.0)
_PRIORITY = {"first": 0, "last": 1}


# ---- host path (numpy) -----------------------------------------------------------------------------------------------------------

def _label_map_np(m, last):
    """m [N,H,W] bool -> int32 [H,W]"""
    N = m.shape[0]
    if N == 0:
        return np.zeros(m.shape[1:], np.int32)
    idx = (N - 1 - np.argmax(m[::-1], 0)) if last else np.argmax(m, 0)           # (argmax: the first maximum)
    return np.where(m.any(0), idx + 1, 0).astype(np.int32)


def _quantise_np(depth_a, depth_b):
    """fp32 arrays -> int64 fixed-point errors (the rule of the module docstring, operation for operation what the kernel does)"""
    da, db = np.asarray(depth_a, np.float32), np.asarray(depth_b, np.float32)
    with np.errstate(invalid="ignore"):
        e = np.abs(db - da)
        e = np.where(da < np.float32(1e-4), np.float32(0), e)
        q = np.rint(np.fmin(e, np.float32(DEPTH_CAP)) * np.float32(DEPTH_SCALE))
    return q.astype(np.int64)


def _overlap_np(la, lb, na, nb, da, db):
    """la, lb int32 [B,H,W] -> (count, wsum) int64 [B,na+1,nb+1]"""
    B = la.shape[0]
    bins = (na + 1) * (nb + 1)
    la, lb = la.reshape(B, -1).astype(np.int64), lb.reshape(B, -1).astype(np.int64)
    ok = (la >= 0) & (la <= na) & (lb >= 0) & (lb <= nb)
    flat = np.where(ok, la * (nb + 1) + lb, 0) + (np.arange(B, dtype=np.int64) * bins)[:, None]
    count = np.bincount(flat[ok], minlength=B * bins).astype(np.int64).reshape(B, na + 1, nb + 1)
    wsum = np.zeros_like(count)
    if da is not None:
        q = _quantise_np(da.reshape(B, -1), db.reshape(B, -1))
        np.add.at(wsum.reshape(-1), flat[ok], q[ok])                                # (integer adds: exact)
    return count, wsum


# ---- label_map ---------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def label_map(masks, priority="first"):
    """Instance masks painted into one label map per image.

    masks     [N,H,W] bool / uint8 tensor (non-zero = set), or a list of per-image tensors (None or N_b = 0: no instances; at least one
              entry must be a tensor: it gives H x W and the device)
    priority  where masks overlap: "first" = the lowest index wins, "last" = the highest
    -> int32 [H,W] (a list: [B,H,W]): 0 = no mask, i + 1 = instance i of that image."""
    if priority not in _PRIORITY:
        raise RuntimeError("label_map: priority must be 'first' or 'last', got %r" % (priority,))
    is_list, parts, ref = _inputs(masks, "label_map")
    if ref is None:
        raise RuntimeError("label_map: every entry of the list is None: H x W is unknown")
    H, W = int(ref.shape[1]), int(ref.shape[2])
    B, dev = len(parts), ref.device
    if not ref.is_cuda:
        maps = [np.zeros((H, W), np.int32) if m is None else _label_map_np(m.numpy().astype(bool), priority == "last") for m in parts]
        out = torch.from_numpy(np.stack(maps))
    elif H * W == 0:
        out = torch.zeros(B, H, W, dtype=torch.int32, device=dev)
    else:
        from ._lib import check, lib
        live = [None if m is None or m.shape[0] == 0 else _as_bytes(m) for m in parts]      # (kept alive until the launch is queued)
        if B == 1:                                                   # one image: no pointer table, nothing to upload
            if live[0] is None:
                return torch.zeros((B, H, W) if is_list else (H, W), dtype=torch.int32, device=dev)
            out = torch.empty(B, H, W, dtype=torch.int32, device=dev)
            check(lib.prn_label_map_flat(_p(live[0]), int(live[0].shape[0]), H, W, _PRIORITY[priority], _p(out), _stream(dev)), "prn_label_map_flat")
            return out if is_list else out[0]
        out = torch.empty(B, H, W, dtype=torch.int32, device=dev)
        first = [0]
        for m in live:
            first.append(first[-1] + (0 if m is None else int(m.shape[0])))
        for b0 in range(0, B, 65535):                                                       # (the grid's y)
            b1 = min(B, b0 + 65535)
            ptrs = _upload([0 if m is None else m.data_ptr() for m in live[b0:b1]], torch.int64, dev)
            firsts = _upload([f - first[b0] for f in first[b0:b1 + 1]], torch.int32, dev)
            check(lib.prn_label_map(_p(ptrs), _p(firsts), b1 - b0, H, W, _PRIORITY[priority], _p(out[b0:]), _stream(dev)), "prn_label_map")
            del ptrs, firsts                                         # (stream-ordered allocator: reuse after this point is ordered behind the launch)
    return out if is_list else out[0]


# ---- overlap -----------------------------------------------------------------------------------------------------------------------

def _check_count(n, what):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= n <= MAX_LABEL:
        raise RuntimeError("overlap: %s must be an integer in [0, %d], got %r" % (what, MAX_LABEL, n))
    return int(n)


@torch.no_grad()
def overlap(labels_a, labels_b, na, nb, depth_a=None, depth_b=None):
    """The overlap tables of two label maps.

    labels_a, labels_b   int32 [H,W] or [B,H,W] (label_map's output), one shape and device
    na, nb               the largest labels, at most 1023: the tables are [na+1, nb+1]; a pixel with a label outside [0, na] / [0, nb] is dropped
    depth_a, depth_b     both or neither: float tensors with the maps' number of elements ([H,W], [1,H,W], [B,1,H,W] ...), a = ground truth
    -> (count, wsum) int64 [na+1, nb+1] (or [B, ...]) on the maps' device: pixels per cell, and the fixed-point sum of |depth_b - depth_a|
       per cell (module docstring; zeros without depths)."""
    na, nb = _check_count(na, "na"), _check_count(nb, "nb")
    for t, what in ((labels_a, "labels_a"), (labels_b, "labels_b")):
        if not (torch.is_tensor(t) and t.dtype == torch.int32 and t.dim() in (2, 3)):
            raise RuntimeError("overlap: %s must be an int32 [H,W] or [B,H,W] tensor, got %s" % (what, _describe(t)))
    if labels_a.shape != labels_b.shape or labels_a.device != labels_b.device:
        raise RuntimeError("overlap: labels_a is %s, labels_b %s (one shape and device)" % (_describe(labels_a), _describe(labels_b)))
    if (depth_a is None) != (depth_b is None):
        raise RuntimeError("overlap: depth_a and depth_b go together")
    single = labels_a.dim() == 2
    la, lb = (t.reshape((-1,) + tuple(t.shape[-2:])).contiguous() for t in (labels_a, labels_b))
    B, H, W = (int(v) for v in la.shape)
    dev = la.device
    if H * W >= 1 << 24:
        raise RuntimeError("overlap: H * W must be below 2^24, got %d x %d" % (H, W))
    depths = [None, None]
    for k, (d, what) in enumerate(((depth_a, "depth_a"), (depth_b, "depth_b"))):
        if d is None:
            continue
        if not (torch.is_tensor(d) and d.is_floating_point() and d.numel() == la.numel() and d.device == dev):
            raise RuntimeError("overlap: %s must be a float tensor with the maps' %d elements on %s, got %s" % (what, la.numel(), dev, _describe(d)))
        depths[k] = d.detach().reshape(B, H, W).float().contiguous()
    if not la.is_cuda:
        c, s = _overlap_np(la.numpy(), lb.numpy(), na, nb, *(None if d is None else d.numpy() for d in depths))
        count, wsum = torch.from_numpy(c), torch.from_numpy(s)
    else:
        tables = torch.zeros(2, B, na + 1, nb + 1, dtype=torch.int64, device=dev)           # (the call adds)
        count, wsum = tables[0], tables[1]
        if B and H * W:
            from ._lib import check, lib
            for b0 in range(0, B, 65535):                                                   # (the grid's y)
                b1 = min(B, b0 + 65535)
                check(lib.prn_label_overlap(_p(la[b0:]), _p(lb[b0:]), *(None if d is None else _p(d[b0:]) for d in depths), b1 - b0, H, W, na, nb,
                                            _p(count[b0:]), _p(wsum[b0:]), _stream(dev)), "prn_label_overlap")
    return (count[0], wsum[0]) if single else (count, wsum)


# ---- scores from the tables (host, fp64) -----------------------------------------------------------------------------------------------

def _entropy_bits(n, N):
    p = n[n > 0] / N
    return float(-(p * np.log2(p)).sum())


def segmentation_scores(T):
    """(RI, VOI, SC) of one frame from its count table T [na+1, nb+1] (rows: ground truth, columns: prediction; row / column 0: no mask),
    over the pixels the ground truth marks planar: row 0 is dropped.  With N = sum T, a_g = sum_p T, b_p = sum_g T:
      RI  = 1 - ((sum a_g^2 + sum b_p^2) / 2 - sum T^2) / (N (N - 1) / 2)                     the Rand index
      VOI = H(a / N) + H(b / N) - 2 MI, in bits; MI = sum over T > 0 of (T / N) log2(T N / (a_g b_p))   the variation of information
      SC  = (sum_g a_g max_p IoU + sum_p b_p max_g IoU) / (2 N), IoU = T / (a_g + b_p - T)      segmentation covering, both directions
    Column 0 -- planar pixels no detection claims -- counts as a segment.  fp64 throughout, no clamp inside the logarithms.  N < 2: NaNs."""
    T = np.asarray(T, dtype=np.int64)[1:].astype(np.float64)
    N = T.sum()
    if T.size == 0 or N < 2:
        return float("nan"), float("nan"), float("nan")
    a, b = T.sum(1), T.sum(0)
    ri = 1.0 - ((np.square(a).sum() + np.square(b).sum()) / 2.0 - np.square(T).sum()) / (N * (N - 1.0) / 2.0)
    nz = T > 0
    outer = a[:, None] * b[None, :]
    mi = float((T[nz] / N * np.log2(T[nz] * N / outer[nz])).sum())
    voi = _entropy_bits(a, N) + _entropy_bits(b, N) - 2.0 * mi
    union = a[:, None] + b[None, :] - T
    iou = np.divide(T, union, out=np.zeros_like(T), where=union > 0)
    sc = float(((a * iou.max(1)).sum() + (b * iou.max(0)).sum()) / (2.0 * N))
    return float(ri), float(voi), sc


def recall_curves(T, S, thresholds=THRESHOLDS, iou=0.5):
    """(plane_recall, pixel_recall) over the depth-error thresholds, PlaneNet's / PlaneRCNN's definitions, from the tables T, S [na+1, nb+1].
    Pairs of real instances only (rows and columns >= 1); areas a_g, b_p over the whole image (row and column 0 included).  A pair
    matches at t iff IoU = T / (a_g + b_p - T) > iou (strict) and its mean error D = S / (T 2^20) <= t (D = 1e6 where T = 0).
      plane recall(t)  the share of ground-truth planes with a matching detection
      pixel recall(t)  sum_g min(sum_p T [match], a_g) / sum_g a_g
    No ground-truth plane: NaNs."""
    T, S = np.asarray(T, dtype=np.int64), np.asarray(S, dtype=np.int64)
    thresholds = np.asarray(thresholds, dtype=np.float64)
    nan = np.full(thresholds.shape, np.nan)
    if T.shape[0] < 2:
        return nan, nan.copy()
    Tf = T.astype(np.float64)
    a, b = Tf.sum(1)[1:], Tf.sum(0)[1:]
    t, s = Tf[1:, 1:], S[1:, 1:].astype(np.float64)
    union = a[:, None] + b[None, :] - t
    good = np.divide(t, union, out=np.zeros_like(t), where=union > 0) > iou
    D = np.where(t > 0, s / (np.maximum(t, 1.0) * DEPTH_SCALE), 1e6)
    match = good[None] & (D[None] <= thresholds[:, None, None])                       # [thresholds, g, p]
    plane = match.any(2).sum(1) / float(a.shape[0])
    total = a.sum()
    covered = np.minimum((t[None] * match).sum(2), a[None]).sum(1)
    pixel = covered / total if total > 0 else nan.copy()
    return plane, pixel


# ---- a whole evaluation run --------------------------------------------------------------------------------------------------------

def _as_masks(m):
    if m is None or m.dtype in (torch.bool, torch.uint8):
        return m
    return m != 0


class PlaneEvalAccumulator:
    """RI / VOI / SC and the recall curves over the frames of an evaluation run.  `add_frame` paints the ground-truth and the predicted masks
    (priority "first") and takes their tables; the tables stay where the masks are.  `result` brings them down in one transfer and scores
    every frame on the host."""

    def __init__(self, thresholds=THRESHOLDS, iou=0.5):
        self.thresholds, self.iou = np.asarray(thresholds, dtype=np.float64), float(iou)
        self._tables = []                                            # per frame: int64 [2, na+1, nb+1]

    def __len__(self):
        return len(self._tables)

    @torch.no_grad()
    def add_frame(self, gt_masks, gt_depth, pred_masks, pred_depth):
        """gt_masks [G,H,W], pred_masks [P,H,W] (None or P = 0: no detections) bool / uint8 (other dtypes: non-zero = set); gt_depth, pred_depth
        float tensors of H * W elements in metres.  At most 1023 instances a side."""
        gt_masks, pred_masks = _as_masks(gt_masks), _as_masks(pred_masks)
        ga = label_map(gt_masks, "first")
        if pred_masks is None or pred_masks.shape[0] == 0:
            pa, nb = torch.zeros_like(ga), 0
        else:
            pa, nb = label_map(pred_masks.to(ga.device), "first"), int(pred_masks.shape[0])
        count, wsum = overlap(ga, pa, int(gt_masks.shape[0]), nb, gt_depth.to(ga.device), pred_depth.to(ga.device))
        self._tables.append(torch.stack([count, wsum]))

    def tables(self):
        """-> [(T, S)] per frame as numpy int64, in one download"""
        if not self._tables:
            return []
        flat = torch.cat([t.reshape(-1) for t in self._tables]).cpu().numpy()
        out, o = [], 0
        for t in self._tables:
            n = t.numel()
            both = flat[o:o + n].reshape(tuple(t.shape))
            out.append((both[0], both[1]))
            o += n
        return out

    def result(self):
        """-> {"RI", "VOI", "SC": frame means; "plane_recall", "pixel_recall": lists over the thresholds; "thresholds"; "frames": frames that
        counted for the scores, "curve_frames": for the curves}.  A frame whose scores are NaN (fewer than two planar pixels, no
        ground-truth plane) is left out of that mean; nothing to average gives NaN."""
        scores, planes, pixels = [], [], []
        for T, S in self.tables():
            scores.append(segmentation_scores(T))
            pl, px = recall_curves(T, S, self.thresholds, self.iou)
            planes.append(pl)
            pixels.append(px)
        scores = np.asarray(scores, dtype=np.float64).reshape(-1, 3)
        ok = ~np.isnan(scores).any(1)
        ri, voi, sc = (scores[ok].mean(0) if ok.any() else np.full(3, np.nan)).tolist()
        planes = np.asarray(planes, dtype=np.float64).reshape(-1, self.thresholds.size)
        pixels = np.asarray(pixels, dtype=np.float64).reshape(-1, self.thresholds.size)
        okc = ~(np.isnan(planes).any(1) | np.isnan(pixels).any(1))
        nanc = np.full(self.thresholds.size, np.nan)
        return {"RI": ri, "VOI": voi, "SC": sc,
                "plane_recall": (planes[okc].mean(0) if okc.any() else nanc).tolist(),
                "pixel_recall": (pixels[okc].mean(0) if okc.any() else nanc).tolist(),
                "thresholds": self.thresholds.tolist(), "frames": int(ok.sum()), "curve_frames": int(okc.sum())}
