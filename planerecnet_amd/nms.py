"""SOLOv2 NMS family on device tensors (reference: models/functions/nms.py). Small tensors; plain device ops."""
import torch
import torch.nn.functional as F


def point_nms(heat, kernel=2):
    """Keep local maxima of a 2x2 window (nms.py:8-12)."""
    assert kernel == 2
    hmax = F.max_pool2d(heat, (2, 2), stride=1, padding=1)
    return heat * (hmax[:, :, :-1, :-1] == heat).float()


def matrix_nms(cate_labels, seg_masks, sum_masks, cate_scores, sigma=2.0, kernel="gaussian"):
    """Parallel soft-NMS by pairwise mask IoU decay (nms.py:15-50)."""
    n = len(cate_labels)
    if n == 0:
        return []
    if seg_masks.is_cuda:
        # pairwise IoU of the bit-packed masks by AND + popcount (include/prn.h: prn_pairwise_iou) instead of an [n, h*w] x [h*w, n]
        # float GEMM: the intersections are the same integers and the quotient inter / ((area_i + area_j) - inter) is formed in the same
        # order, so the matrix is bit-identical (tests/test_eval_metrics.py pins the kernel on the reference's float matmul)
        from .metrics import mask_iou, matrix_nms_scores
        iou = mask_iou(seg_masks, seg_masks)
        if kernel in ("gaussian", "linear"):
            # the decay of the scores from the IoU matrix in two launches (prn_matrix_nms): the same operations per element as the dense form below
            return matrix_nms_scores(iou, cate_labels, cate_scores, float(sigma), kernel == "gaussian")
        iou = iou.triu(diagonal=1)
    else:
        flat = seg_masks.reshape(n, -1).float()
        inter = flat @ flat.t()
        area = sum_masks.expand(n, n)
        iou = (inter / (area + area.t() - inter)).triu(diagonal=1)
    lab = cate_labels.expand(n, n)
    decay = iou * (lab == lab.t()).float().triu(diagonal=1)
    comp = decay.max(0)[0].expand(n, n).t()
    if kernel == "linear":
        coef = ((1 - decay) / (1 - comp)).min(0)[0]
    else:
        coef = (torch.exp(-sigma * decay ** 2) / torch.exp(-sigma * comp ** 2)).min(0)[0]
    return cate_scores * coef


MASK_NMS_MAX = 4096      # candidates per image (include/prn.h: PRN_MASK_NMS_MAX)


def mask_nms_batched(cate_labels, seg_masks, sum_masks, counts, nms_thr=0.5):
    """Greedy mask NMS (nms.py:53-81) of a ragged batch in one call (include/prn.h: prn_mask_nms; csrc/prn_mask_nms.hip).  cate_labels [N],
    seg_masks [N,h,w] (bool / uint8; another dtype counts as != 0), sum_masks [N]: device tensors, the candidates of image b contiguous and in
    descending score order; counts: host ints per image (zeros allowed, sum N).  -> keep [N] in seg_masks.dtype.  One small upload (the segment
    offsets, through page-locked memory), one workspace, three launches, no host synchronisation."""
    from ._lib import check, lib
    from ._masks import _p as p, _stream, _upload
    if not (seg_masks.is_cuda and cate_labels.is_cuda and sum_masks.is_cuda):
        raise RuntimeError("mask_nms_batched needs device tensors (CPU tensors: mask_nms)")
    counts = [int(c) for c in counts]
    N = int(seg_masks.shape[0])
    if any(c < 0 for c in counts) or sum(counts) != N or cate_labels.shape[0] != N or sum_masks.shape[0] != N:
        raise RuntimeError("mask_nms_batched: counts %s do not add up to the %d masks / %d labels / %d sums given"
                           % (counts, N, cate_labels.shape[0], sum_masks.shape[0]))
    n_max = max(counts) if counts else 0
    if n_max > MASK_NMS_MAX:
        raise RuntimeError("mask_nms_batched: %d candidates in one image, the limit is %d" % (n_max, MASK_NMS_MAX))
    dev = seg_masks.device
    keep = torch.empty(N, device=dev, dtype=torch.uint8)
    if N == 0:
        return keep.to(seg_masks.dtype)
    HW = int(seg_masks[0].numel())
    masks = (seg_masks if seg_masks.dtype in (torch.uint8, torch.bool) else seg_masks != 0).contiguous().view(torch.uint8)
    labels, sums = cate_labels.long().contiguous(), sum_masks.float().contiguous()
    offsets = [0]
    for c in counts:
        offsets.append(offsets[-1] + c)
    seg = _upload(offsets, torch.int32, dev)
    ws = torch.empty((lib.prn_mask_nms_ws_bytes(N, n_max, HW) + 7) // 8 * 2, device=dev, dtype=torch.float32)
    stream = _stream(dev)
    check(lib.prn_mask_nms(p(masks), p(labels), p(sums), p(seg), len(counts), n_max, HW, float(nms_thr), p(keep), p(ws), stream), "prn_mask_nms")
    return keep.to(seg_masks.dtype)


def mask_nms(cate_labels, seg_masks, sum_masks, cate_scores, nms_thr=0.5):
    """Greedy mask NMS (nms.py:53-81).  Device tensors: mask_nms_batched with one segment.  CPU tensors: the pairwise IoU matrix computed once
    instead of per pair, then the reference's double loop."""
    n = len(cate_scores)
    if n == 0:
        return []
    if seg_masks.is_cuda:
        return mask_nms_batched(cate_labels, seg_masks, sum_masks, [n], nms_thr=nms_thr)
    flat = seg_masks.reshape(n, -1).float()
    inter = flat @ flat.t()
    union = sum_masks[:, None] + sum_masks[None, :] - inter
    same = cate_labels[:, None] == cate_labels[None, :]
    suppress = same & ((union <= 0) | (inter / union.clamp(min=1e-12) > nms_thr))
    keep = [True] * n
    for i in range(n - 1):
        if keep[i]:
            for j in range(i + 1, n):
                if keep[j] and suppress[i, j]:
                    keep[j] = False
    return torch.tensor(keep, device=seg_masks.device).to(seg_masks.dtype)
