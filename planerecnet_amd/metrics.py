"""Evaluation metrics (reference eval.py:164-354): `compute_depth_metrics` and the detection metrics
(`compute_segmentation_metrics`, `APDataObject`, `calc_map`), the latter further down.

Depth errors:

Same signature and return tuple as the reference function: (abs_rel, sq_rel, rmse, log10, a1, a2, a3, ratio) as CPU
tensors.  The seven error terms come from ONE fused HIP reduction (include/prn.h: prn_depth_metrics); the median ratio is
computed as in the reference (median of ALL ground-truth depths over the median of the valid predictions, eval.py:184 --
reported only, the prediction is not rescaled).
"""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from ._lib import check, lib
from ._masks import _p, _stream
from .config import cfg


def compute_depth_metrics(pred_depth, gt_depth, median_scaling=True):
    """pred_depth, gt_depth: [1, H, W] dense depth maps in the same unit (device tensors)."""
    if not (pred_depth.is_cuda and gt_depth.is_cuda):
        raise RuntimeError("compute_depth_metrics needs device tensors; there is no CPU path in the product")
    pred = pred_depth.detach().float().contiguous()
    gt = gt_depth.detach().float().contiguous()
    if pred.numel() != gt.numel():
        raise RuntimeError("compute_depth_metrics: prediction %s and ground truth %s differ in size" % (tuple(pred.shape), tuple(gt.shape)))
    out = torch.empty(8, device=pred.device, dtype=torch.float64)
    ws = torch.empty(lib.prn_depth_metrics_ws_doubles(), device=pred.device, dtype=torch.float64)
    stream = _stream(pred.device)
    check(lib.prn_depth_metrics(_p(pred), _p(gt), _p(out), _p(ws), pred.numel(), float(cfg.dataset.min_depth), float(cfg.dataset.max_depth), stream),
          "prn_depth_metrics")
    if median_scaling:
        valid = (gt.flatten() > 0.5).logical_and(pred.flatten() > 0.5)
        ratio = (torch.median(gt) / torch.median(pred.flatten()[valid])).cpu()
    else:
        ratio = torch.tensor(0)
    o = out.cpu()
    return o[0], o[1], o[2], o[3], o[4], o[5], o[6], ratio


# ---------------------------------------------------------------------------------------------------------------------------
# Detection metrics (reference eval.py:210-354).  The pairwise IoU matrices of a frame come from the device
# (include/prn.h: prn_pairwise_iou -- bit-packed masks, AND + popcount); the per-threshold matching and the AP integral are a
# few hundred scalar operations per frame and stay on the host, vectorised, with the reference's exact outcomes (including
# its quirks, see compute_segmentation_metrics).
iou_thresholds = [x / 100 for x in range(50, 100, 5)]                                   # eval.py:61
depth_metrics = ["abs_rel", "sq_rel", "rmse", "log10", "a1", "a2", "a3", "ratio"]      # eval.py:60


def pairwise_iou(masks_a=None, masks_b=None, boxes_a=None, boxes_b=None):
    """-> (mask_iou [A,B] | None, box_iou [A,B] | None), fp32 device tensors.  masks: [A,H,W] / [B,H,W], any dtype, non-zero = set
    (the reference multiplies their 0/1 float copies); boxes: [A,4] / [B,4] (x1,y1,x2,y2), converted to fp32 like eval.py:215."""
    ref = masks_a if masks_a is not None else boxes_a
    if ref is None or not ref.is_cuda:
        raise RuntimeError("pairwise_iou needs device tensors; there is no CPU path in the product")
    dev = ref.device
    A = ref.shape[0]
    B = (masks_b if masks_a is not None else boxes_b).shape[0]
    want_m, want_b = masks_a is not None, boxes_a is not None
    if A == 0 or B == 0:
        e = torch.empty(A, B, device=dev)
        return (e if want_m else None), (e.clone() if want_b else None)
    HW, ma, mb, miou, ws = 1, None, None, None, None
    if want_m:
        if masks_a.shape[1:] != masks_b.shape[1:]:
            raise RuntimeError("pairwise_iou: mask sets of different size %s / %s" % (tuple(masks_a.shape), tuple(masks_b.shape)))
        HW = int(masks_a[0].numel())
        ma = (masks_a if masks_a.dtype in (torch.uint8, torch.bool) else masks_a != 0).contiguous().view(torch.uint8)
        mb = (masks_b if masks_b.dtype in (torch.uint8, torch.bool) else masks_b != 0).to(dev).contiguous().view(torch.uint8)
        miou = torch.empty(A, B, device=dev)
        ws = torch.empty(lib.prn_pairwise_iou_ws_bytes(A, B, HW), device=dev, dtype=torch.uint8)
    ba = bb = biou = None
    if want_b:
        ba, bb = boxes_a.to(dev).float().contiguous(), boxes_b.to(dev).float().contiguous()
        biou = torch.empty(A, B, device=dev)
    stream = _stream(dev)
    check(lib.prn_pairwise_iou(_p(ma), _p(mb), _p(ba), _p(bb), A, B, HW, _p(miou), _p(biou), _p(ws), stream), "prn_pairwise_iou")
    return miou, biou


def boundary_iou(masks_a, masks_b, radius=None, ratio=0.02):
    """-> (mask_iou [A,B], boundary_iou [A,B]), fp32 device tensors, from one call (include/prn.h: prn_boundary_iou).  masks as for
    `pairwise_iou`.  boundary_iou is the IoU of the inner bands m & ~erode(m, radius, border=0) (morphology.boundary; Cheng et al., CVPR
    2021), which are built and compared bit-packed; mask_iou is bit-identical to pairwise_iou's.  radius=None: morphology.boundary_radius
    of the mask size with `ratio`.  A pair of empty masks gives NaN in both."""
    from .morphology import _check, boundary_radius
    if not (torch.is_tensor(masks_a) and torch.is_tensor(masks_b) and masks_a.is_cuda and masks_a.dim() == 3 and masks_b.dim() == 3):
        raise RuntimeError("boundary_iou needs [A,H,W] / [B,H,W] device tensors; there is no CPU path in the product")
    if masks_a.shape[1:] != masks_b.shape[1:]:
        raise RuntimeError("boundary_iou: mask sets of different size %s / %s" % (tuple(masks_a.shape), tuple(masks_b.shape)))
    dev = masks_a.device
    A, B, H, W = int(masks_a.shape[0]), int(masks_b.shape[0]), int(masks_a.shape[1]), int(masks_a.shape[2])
    radius = boundary_radius(H, W, ratio) if radius is None else _check(radius, 0, "boundary_iou", tuple(masks_a.shape))[0]
    if A == 0 or B == 0:
        return torch.empty(A, B, device=dev), torch.empty(A, B, device=dev)
    nbytes = lib.prn_boundary_iou_ws_bytes(A, B, H, W)
    if nbytes < 0:
        raise RuntimeError("boundary_iou: needs 1 <= A, B < 65536 and 0 < H * W < 2^24, got %s / %s" % (tuple(masks_a.shape), tuple(masks_b.shape)))
    ma = (masks_a if masks_a.dtype in (torch.uint8, torch.bool) else masks_a != 0).contiguous().view(torch.uint8)
    mb = (masks_b if masks_b.dtype in (torch.uint8, torch.bool) else masks_b != 0).to(dev).contiguous().view(torch.uint8)
    out = torch.empty(2, A, B, device=dev)
    ws = torch.empty((nbytes + 7) // 8 * 2, device=dev, dtype=torch.int32)
    stream = _stream(dev)
    check(lib.prn_boundary_iou(_p(ma), _p(mb), A, B, H, W, radius, _p(out[0]), _p(out[1]), _p(ws), stream), "prn_boundary_iou")
    return out[0], out[1]


def category_scores(cate_logits):
    """list of [B, C, S, S] category logits (one per grid level) -> [B, cells, C] scores after sigmoid + 2x2 point NMS, levels concatenated
    (reference planerecnet.py:113 + models/functions/nms.py:8-12 + the level concatenation of `inference`), one launch per level."""
    B, C = cate_logits[0].shape[:2]
    cells = sum(int(c.shape[2]) * int(c.shape[3]) for c in cate_logits)
    out = torch.empty(B, cells, C, device=cate_logits[0].device, dtype=torch.float32)
    stream = _stream(out.device)
    off = 0
    for c in cate_logits:
        S = int(c.shape[2])
        if not c.is_cuda or c.dtype != torch.float32 or c.shape[3] != S or c.shape[:2] != (B, C):
            raise RuntimeError("category_scores needs square fp32 device maps of one batch / class count")
        c = c.detach().contiguous()
        check(lib.prn_sigmoid_point_nms(_p(c), ctypes.c_void_p(out.data_ptr() + 4 * off * C), B, C, S, cells * C, stream), "prn_sigmoid_point_nms")
        off += S * S
    return out


def mask_stats(seg, thr):
    """[n,h,w] soft masks -> (count [n], msum [n]) of the values above thr, fp32 (include/prn.h: prn_mask_stats)."""
    if not seg.is_cuda or seg.dtype != torch.float32:
        raise RuntimeError("mask_stats needs fp32 device tensors")
    n = seg.shape[0]
    out = torch.empty(2, n, device=seg.device, dtype=torch.float32)
    if n:
        seg = seg.contiguous()
        stream = _stream(seg.device)
        check(lib.prn_mask_stats(_p(seg), n, int(seg[0].numel()), float(thr), _p(out[0]), _p(out[1]), stream), "prn_mask_stats")
    return out[0], out[1]


def mask_boxes(masks):
    """[n,H,W] binary masks (bool / uint8, on the device) -> [n,4] float (x0, y0, x1, y1) of their set pixels, one launch
    (reference planerecnet.py:282-287; an empty mask gives (H+W, H+W, -1, -1) like the vectorised torch form)."""
    if not masks.is_cuda or masks.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError("mask_boxes needs bool / uint8 device masks")
    n, H, W = masks.shape
    out = torch.empty(n, 4, device=masks.device, dtype=torch.float32)
    if n:
        m = masks.contiguous().view(torch.uint8)
        stream = _stream(masks.device)
        check(lib.prn_mask_boxes(_p(m), n, H, W, _p(out), stream), "prn_mask_boxes")
    return out


def matrix_nms_scores(iou, labels, scores, sigma, gaussian):
    """Matrix-NMS decayed scores from the [n, n] mask-IoU matrix of detections in descending score order (include/prn.h: prn_matrix_nms)."""
    n = scores.shape[0]
    iou, labels, scores = iou.contiguous(), labels.contiguous().long(), scores.contiguous().float()
    out = torch.empty(2, n, device=scores.device, dtype=torch.float32)          # decayed scores | workspace (per-column denominators)
    stream = _stream(scores.device)
    check(lib.prn_matrix_nms(_p(iou), _p(labels), _p(scores), n, float(sigma), int(bool(gaussian)), _p(out[0]), _p(out[1]), stream), "prn_matrix_nms")
    return out[0]


def mask_iou(masks_a, masks_b, iscrowd=False):
    """[a,h,w] x [b,h,w] -> [a,b]  (reference models/functions/funcs.py:58-71)."""
    if iscrowd:
        raise NotImplementedError("mask_iou(iscrowd=True) has no call site in the reference and is not built")
    return pairwise_iou(masks_a=masks_a, masks_b=masks_b)[0]


def bbox_iou(box_a, box_b):
    """[A,4] x [B,4] -> [A,B]  (reference models/functions/funcs.py:30-56, the un-batched form eval.py uses)."""
    if box_a.dim() != 2:
        raise NotImplementedError("bbox_iou: the batched [n,A,4] form has no call site in the reference and is not built")
    return pairwise_iou(boxes_a=box_a, boxes_b=box_b)[1]


class APDataObject:
    """Scores and hit flags of the detections seen for one IoU threshold and one class (reference eval.py:254-325)."""

    def __init__(self):
        self.scores, self.hits = [], []
        self.num_gt_positives = 0

    def push(self, score, is_true):
        self.scores.append(float(score))
        self.hits.append(bool(is_true))

    def extend(self, scores, hits):
        self.scores.extend(scores)
        self.hits.extend(hits)

    def add_gt_positives(self, num_positives):
        self.num_gt_positives += num_positives

    def is_empty(self):
        return len(self.scores) == 0 and self.num_gt_positives == 0

    def get_ap(self):
        """101-point interpolated AP: precision envelope sampled at recall 0, 0.01, ..., 1 (eval.py:272-325)."""
        if self.num_gt_positives == 0:
            return 0
        n = len(self.scores)
        if n == 0:
            return 0.0
        order = np.argsort(-np.asarray(self.scores, np.float64), kind="stable")       # equal scores keep their push order
        hit = np.asarray(self.hits, bool)[order]
        tp, fp = np.cumsum(hit), np.cumsum(~hit)
        prec = tp / (tp + fp)
        rec = tp / self.num_gt_positives
        prec = np.maximum.accumulate(prec[::-1])[::-1]
        idx = np.searchsorted(rec, np.array([x / 100 for x in range(101)]), side="left")
        bars = np.where(idx < n, prec[np.minimum(idx, n - 1)], 0.0)
        return sum(bars.tolist()) / 101                                               # left-to-right like the reference's sum()


def new_ap_data(boundary=False):
    """boundary: a third list "boundary" (Boundary AP: a detection matches iff min(mask IoU, boundary IoU) exceeds the threshold)"""
    data = {"box": [APDataObject() for _ in iou_thresholds], "mask": [APDataObject() for _ in iou_thresholds]}     # eval.py:77-80
    if boundary:
        data["boundary"] = [APDataObject() for _ in iou_thresholds]
    return data


def match_frame(ap_data, mask_iou_np, box_iou_np, scores, num_gt_for_class, boundary_iou_np=None):
    """Host half of compute_segmentation_metrics: push one frame's detections into `ap_data` given its [A,B] IoU matrices.
    boundary_iou_np: also push the "boundary" objects, matched on min(mask IoU, boundary IoU) (COCO's Boundary AP; NaN never matches)."""
    scores = np.asarray(scores, np.float64)
    order = np.argsort(-scores, kind="stable")                                        # eval.py:217
    s = scores[order]
    kinds = (("box", box_iou_np), ("mask", mask_iou_np))
    if boundary_iou_np is not None:
        kinds += (("boundary", np.minimum(mask_iou_np, boundary_iou_np)),)
    for t, thr in enumerate(iou_thresholds):
        for kind, iou in kinds:
            obj = ap_data[kind][t]
            obj.add_gt_positives(num_gt_for_class)
            matched = (iou[order] > thr).any(axis=1) if iou.shape[1] else np.zeros(len(order), bool)    # NaN (empty masks) never matches
            # every detection is pushed as a miss, a matched one as a hit before it (eval.py:248-252)
            reps = 1 + matched.astype(np.int64)
            flags = np.zeros(int(reps.sum()), bool)
            flags[(np.cumsum(reps) - reps)[matched]] = True
            obj.extend(np.repeat(s, reps).tolist(), flags.tolist())


def compute_segmentation_metrics(ap_data, gt_masks, gt_boxes, gt_classes, pred_masks, pred_boxes, pred_classes, pred_scores, boundary_radius=None):
    """One frame's detections against its ground truth, for every IoU threshold, boxes and masks (reference eval.py:210-252;
    same argument list).  Two reference behaviours are kept on purpose: a matched detection counts as a hit AND as a miss, and
    one ground-truth instance may be matched by several detections.
    boundary_radius: also push the "boundary" objects of `ap_data` (new_ap_data(boundary=True)); the mask IoU then comes with the
    boundary IoU from one prn_boundary_iou call, the box IoU from prn_pairwise_iou as before."""
    num_gt_for_class = int((torch.as_tensor(gt_classes) == 0).sum())                  # eval.py:234
    scores = torch.as_tensor(pred_scores).detach().cpu().numpy()
    if boundary_radius is None:
        miou, biou = pairwise_iou(pred_masks, gt_masks.to(pred_masks.device), pred_boxes, gt_boxes)
        match_frame(ap_data, miou.cpu().numpy(), biou.cpu().numpy(), scores, num_gt_for_class)
        return
    miou, bdiou = boundary_iou(pred_masks, gt_masks.to(pred_masks.device), radius=boundary_radius)
    biou = pairwise_iou(boxes_a=pred_boxes.to(pred_masks.device), boxes_b=gt_boxes)[1]
    match_frame(ap_data, miou.cpu().numpy(), biou.cpu().numpy(), scores, num_gt_for_class, boundary_iou_np=bdiou.cpu().numpy())


def calc_map(ap_data, quiet=False):
    """-> {'box': {'all', 50, 55, ..., 95}, 'mask': {...}} in percent, rounded to two decimals (reference eval.py:327-354); a 'boundary' row
    iff `ap_data` has the key."""
    if not quiet:
        print("Calculating mAP...")
    all_maps = {}
    for kind in ("box", "mask") + (("boundary",) if "boundary" in ap_data else ()):
        row = OrderedDict([("all", 0)])
        for t, thr in enumerate(iou_thresholds):
            obj = ap_data[kind][t]
            row[int(thr * 100)] = obj.get_ap() * 100 if not obj.is_empty() else 0
        row["all"] = sum(row.values()) / (len(row) - 1)
        all_maps[kind] = row
    if not quiet:
        print_maps(all_maps)
    return {k: {j: round(u, 2) for j, u in v.items()} for k, v in all_maps.items()}


def print_maps(all_maps):
    """The reference's table layout (eval.py:356-370); the 'boundary' row, where there is one, is labelled 'bndry' (the cell is five wide)."""
    keys = list(all_maps["box"].keys())
    cell = " %5s |"
    rule = "-------+" * (len(keys) + 1)
    print()
    print(cell * (len(keys) + 1) % tuple([""] + [(".%d " % k) if isinstance(k, int) else k + " " for k in keys]))
    print(rule)
    for kind in ("box", "mask") + (("boundary",) if "boundary" in all_maps else ()):
        name = "bndry" if kind == "boundary" else kind
        print(cell * (len(keys) + 1) % tuple([name] + [("%.2f" % v) if v < 100 else ("%.1f" % v) for v in all_maps[kind].values()]))
    print(rule)
    print()
