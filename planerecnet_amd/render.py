"""The inference overlay and the depth picture, drawn on the device (include/prn.h: prn_render_*).

simple_inference.py draws on the host: every [N,H,W] mask and the float frame are downloaded, one full-frame `np.where` runs per
detection, the depth map is sorted twice for its 1 % / 99 % limits.  Here the overlay is one HIP launch over the mask bytes, the limits
a radix select (no sort, integer histograms only) and the colouring one pass; what comes back to the host is one uint8 image each.
None of the functions synchronises the host.

Pinned on the host code of simple_inference.py (`display_on_frame` with no_text, `_viridis`), bit for bit: the blend
`v = fl32(fl32(v * fl32(1 - alpha)) + fl32(colour * fl32(alpha)))` from the last detection down and the truncation to uint8, the box
outlines (Pillow's `rectangle(outline, width=1)`), the 256 colour levels.  Deviations:
  * a box with y0 == y1 is ONE row here; Pillow draws a second row below it.
  * the mask outlines (`contours=True`; the reference: findContours / drawContours in white) are defined as: a pixel of mask i any of
    whose four neighbours is outside mask i or outside the image becomes white.  That is what a one-pixel drawContours covers as far as
    its documentation goes; OpenCV is not a dependency of this build, so the rule is NOT pinned on OpenCV's output.
  * out-of-range frame values saturate to [0, 255] (numpy's cast wraps); frames from `frame_to_input` are inside the range.
"""
import numpy as np
import torch

from ._lib import check, lib
from ._masks import _as_bytes, _describe, _p, _stream, _upload
from .config import COLORS

__all__ = ["render_overlay", "depth_limits", "colorize_depth", "viridis_table", "LAYER_MASKS", "LAYER_CONTOURS", "LAYER_BOXES"]

LAYER_MASKS, LAYER_CONTOURS, LAYER_BOXES = 1, 2, 4           # PRN_RENDER_* of include/prn.h
_BOX_LIMIT = 1 << 30                                         # boxes further out than this are clamped (no image is that large)
_VIRIDIS_STOPS = [0, 64, 128, 192, 255]
_VIRIDIS_RGB = ([68, 59, 33, 94, 253], [1, 82, 145, 201, 231], [84, 139, 140, 98, 37])
_TABLES = {}                                                 # device -> the viridis table there (BGR)


def viridis_table():
    """the 256 colours of simple_inference._viridis as uint8 [256,3] RGB: the 5-stop ramp interpolated at every level, truncated"""
    levels = np.arange(256)
    return np.stack([np.interp(levels, _VIRIDIS_STOPS, c) for c in _VIRIDIS_RGB], -1).astype(np.uint8)


def box_table(boxes, n, check_order=True):
    """pred_boxes (a HOST tensor [n,4], x0 y0 x1 y1) -> n lists of four ints, truncated with int() like the host drawing; reversed
    boxes raise ValueError as Pillow's rectangle does"""
    if not torch.is_tensor(boxes) or boxes.is_cuda:
        raise RuntimeError("pred_boxes must be a host tensor (the model returns it on the CPU), got %s" % _describe(boxes))
    if boxes.dim() != 2 or tuple(boxes.shape) != (n, 4):
        raise RuntimeError("pred_boxes must be [%d,4] (one box per mask), got %s" % (n, tuple(boxes.shape)))
    table = []
    for row in boxes.tolist():
        x0, y0, x1, y1 = [max(-_BOX_LIMIT, min(_BOX_LIMIT, int(v))) for v in row]
        if check_order and x1 < x0:
            raise ValueError("x1 must be greater than or equal to x0")
        if check_order and y1 < y0:
            raise ValueError("y1 must be greater than or equal to y0")
        table.append([x0, y0, x1, y1])
    return table


def color_table(n):
    """the colour of detection i, as the host drawing picks it: COLORS[(i * 5) % len(COLORS)], stored RGB -> BGR"""
    return [list(COLORS[(i * 5) % len(COLORS)][::-1]) for i in range(n)]


@torch.no_grad()
def render_overlay(result, frame, mask_alpha=0.5, no_mask=False, no_box=False, contours=False):
    """Masks, mask outlines and boxes of one eval-mode result dict over the frame, in one launch.

    result  {"pred_masks": [N,H,W] bool / uint8 device tensor, "pred_boxes": [N,4] HOST tensor, "pred_scores": ...}; `pred_scores` None
            (no detections) or N == 0 gives the truncated frame
    frame   [H,W,3] fp32 BGR device tensor (what funcs.frame_to_input returns beside the batch)
    -> uint8 [H,W,3] BGR device tensor: simple_inference.display_on_frame(..., no_text=True) bit for bit (module docstring: deviations);
       `contours=True` adds the white one-pixel mask outlines between the blend and the boxes.
    Neither the dict nor its tensors are modified."""
    if not (torch.is_tensor(frame) and frame.dtype == torch.float32 and frame.dim() == 3 and frame.shape[2] == 3):
        raise RuntimeError("frame must be a [H,W,3] fp32 device tensor, got %s" % _describe(frame))
    H, W = int(frame.shape[0]), int(frame.shape[1])
    if H == 0 or W == 0:
        raise RuntimeError("frame must not be empty, got %s" % (tuple(frame.shape),))
    masks = result.get("pred_masks")
    n = 0 if result.get("pred_scores") is None or masks is None else int(masks.shape[0])
    boxes = None
    if n:
        if not (torch.is_tensor(masks) and masks.dtype in (torch.bool, torch.uint8) and masks.dim() == 3 and tuple(masks.shape[1:]) == (H, W)):
            raise RuntimeError("pred_masks must be a bool / uint8 [N,%d,%d] tensor, got %s" % (H, W, _describe(masks)))
        boxes = box_table(result.get("pred_boxes"), n, check_order=not no_box)
    if not frame.is_cuda:
        raise RuntimeError("frame must be a [H,W,3] fp32 device tensor, got %s" % _describe(frame))
    dev = frame.device
    if n and masks.device != dev:
        raise RuntimeError("pred_masks must be on %s like the frame, got %s" % (dev, masks.device))
    layers = (0 if no_mask else LAYER_MASKS) | (LAYER_CONTOURS if contours else 0) | (0 if no_box else LAYER_BOXES)
    frame = frame.contiguous()
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    m = colors_dev = boxes_dev = None
    if n:
        m = _as_bytes(masks)
        colors_dev = _upload(color_table(n), torch.uint8, dev)
        boxes_dev = _upload(boxes, torch.int32, dev)
    alpha, one_minus = float(np.float32(mask_alpha)), float(np.float32(1 - mask_alpha))      # (the subtraction in double first, as the host code)
    check(lib.prn_render_overlay(_p(frame), _p(m), _p(colors_dev), _p(boxes_dev), n, H, W, alpha, one_minus, layers, _p(out), _stream(dev)),
          "prn_render_overlay")
    return out


def _depth_map(depth):
    if not (torch.is_tensor(depth) and depth.dtype == torch.float32):
        raise RuntimeError("depth must be a fp32 device tensor, got %s" % _describe(depth))
    if depth.numel() == 0 or depth.numel() >= 1 << 31:
        raise RuntimeError("depth must hold between 1 and 2^31 - 1 values, got %s" % (tuple(depth.shape),))
    if not depth.is_cuda:
        raise RuntimeError("depth must be a fp32 device tensor, got %s" % _describe(depth))
    return depth.contiguous()


@torch.no_grad()
def depth_limits(depth, q=(1, 99)):
    """The q[0] % and q[1] % limits of a depth map over its non-NaN values (np.nanpercentile's linear rule), without a sort.

    depth  fp32 device tensor of any shape
    -> fp32 [8] device tensor { vmin, vmax, lo_a, lo_b, hi_a, hi_b, min, max }: the two limits; the order statistics next to the
       virtual indices (count - 1) * q / 100, exact (vmin = lo_a + (lo_b - lo_a) * fraction in fp64, rounded to fp32); the non-NaN
       minimum and maximum.  A map of nothing but NaN gives eight zeros.  Deterministic (integer histograms only)."""
    if len(q) != 2 or not all(0 <= float(v) <= 100 for v in q):
        raise ValueError("q must be two percentages in [0, 100], got %r" % (q,))
    d = _depth_map(depth)
    limits = torch.empty(8, dtype=torch.float32, device=d.device)
    ws = torch.empty(lib.prn_render_limits_ws_bytes(), dtype=torch.uint8, device=d.device)
    check(lib.prn_render_depth_limits(_p(d), d.numel(), float(q[0]) / 100, float(q[1]) / 100, _p(limits), _p(ws), _stream(d.device)),
          "prn_render_depth_limits")
    return limits


@torch.no_grad()
def colorize_depth(depth, limits=None, mode="colored", depth_shift=512):
    """The depth picture of simple_inference.py on the device.

    depth   fp32 device tensor holding one [H,W] map (leading dimensions of size 1 are dropped)
    mode    "colored": the map clipped to its limits, stretched to 256 levels and sent through the viridis table -> uint8 [H,W,3] BGR
            (simple_inference._viridis with those limits, bit for bit; NaN -> level 0); limits: what depth_limits returned for this map
            (None: computed here, 1 % / 99 %)
            "gray": uint16 [H,W] = trunc(depth * depth_shift), saturated to [0, 65535], NaN -> 0"""
    if mode not in ("colored", "gray"):
        raise ValueError("mode must be 'colored' or 'gray', got %r" % (mode,))
    if not torch.is_tensor(depth) or depth.dim() < 2 or depth.numel() != depth.shape[-2] * depth.shape[-1]:
        raise RuntimeError("depth must hold one [H,W] map, got %s" % _describe(depth))
    d = _depth_map(depth)
    H, W = int(d.shape[-2]), int(d.shape[-1])
    dev = d.device
    if mode == "gray":
        out = torch.empty(H, W, dtype=torch.uint16, device=dev)
        check(lib.prn_render_depth_gray(_p(d), d.numel(), float(depth_shift), _p(out), _stream(dev)), "prn_render_depth_gray")
        return out
    if limits is None:
        limits = depth_limits(d)
    elif not (torch.is_tensor(limits) and limits.device == dev and limits.dtype == torch.float32 and tuple(limits.shape) == (8,)):
        raise RuntimeError("limits must be the fp32 [8] tensor depth_limits returned on %s, got %s" % (dev, _describe(limits)))
    if dev not in _TABLES:
        _TABLES[dev] = _upload(viridis_table()[:, ::-1].tolist(), torch.uint8, dev)
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    check(lib.prn_render_depth_colors(_p(d), d.numel(), _p(limits.contiguous()), _p(_TABLES[dev]), _p(out), _stream(dev)), "prn_render_depth_colors")
    return out
