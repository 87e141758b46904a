"""Plane parameters of detected instances and the planar depth map (include/prn.h: prn_planes_*).

The reference derives them only in its iBims-1 "plane depth" exporter (simple_inference.py:240-324): per instance, the depth
under the mask back-projected with the intrinsics K, the plane through the centroid normal to the smallest principal axis
(PCA_svd, models/functions/funcs.py:287-291), and the depth inside the mask replaced by that plane's ray-intersection depth,
the highest-index instance winning where masks overlap.  Here a whole ragged batch is three HIP launches and no host
synchronisation (sizes come from tensor shapes, which the host knows).

Deviations where the reference crashes or returns an arbitrary plane: an instance with fewer than 3 pixels or collinear points
(a degenerate scatter) is INVALID -- NaN plane, no part in the composition (its pixels take the next valid covering instance
below it, or keep the predicted depth).  The reference raises on a 1-pixel mask (`squeeze` turns the [1,3] point set into a
vector) and returns an arbitrary plane for 2 pixels.
"""
import torch

from ._lib import check, lib
from ._masks import _as_bytes, _describe, _p, _stream, _upload

__all__ = ["fit_planes", "fit_planes_ransac", "planar_depth"]


def _intrinsics(k_matrix, B, device):
    """K as [3,3] or [B,3,3] (tensor anywhere or array) -> [B,9] fp64 on the device"""
    k = torch.as_tensor(k_matrix)
    if k.shape not in ((3, 3), (B, 3, 3)):
        raise RuntimeError("k_matrix must be [3,3] or [B,3,3] (B=%d), got %s" % (B, tuple(k.shape)))
    if k.is_cuda:
        k = k.to(device=device, dtype=torch.float64)
    else:
        k = k.to(torch.float64).contiguous().pin_memory().to(device, non_blocking=True)
    return k.expand(B, 3, 3).reshape(B, 9).contiguous()


class _Fit:
    """one prn_planes_fit call: its device tables, outputs and workspace (the render launch reads the same workspace);
    lsq=False: the checked inputs and device tables only (what fit_planes_ransac needs)"""

    def __init__(self, depth, masks, k_matrix, lsq=True):
        if not (torch.is_tensor(depth) and depth.is_cuda and depth.dtype == torch.float32 and depth.dim() == 4 and depth.shape[1] == 1):
            raise RuntimeError("depth must be a [B,1,H,W] fp32 device tensor, got %s" % _describe(depth))
        B, _, H, W = depth.shape
        dev = depth.device
        if len(masks) != B:
            raise RuntimeError("masks: one [N,H,W] tensor per image expected (%d images, %d mask tensors)" % (B, len(masks)))
        ms = []
        for b, m in enumerate(masks):
            if m is None:
                m = torch.zeros(0, H, W, dtype=torch.uint8, device=dev)
            if not (m.device == dev and m.dtype in (torch.bool, torch.uint8) and m.dim() == 3 and tuple(m.shape[1:]) == (H, W)):
                raise RuntimeError("masks[%d] must be a bool / uint8 [N,%d,%d] tensor on %s, got %s %s %s" % (b, H, W, dev, m.device, m.dtype, tuple(m.shape)))
            ms.append(_as_bytes(m))
        self.sizes = [int(m.shape[0]) for m in ms]
        first = [0]
        for n in self.sizes:
            first.append(first[-1] + n)
        self.B, self.H, self.W, self.Ntot = B, H, W, first[-1]
        self.depth = depth.contiguous()
        self.masks = ms                                          # (kept alive with the pointer table)
        self.given = list(masks)
        self.ptrs = _upload([m.data_ptr() for m in ms], torch.int64, dev)
        self.first = _upload(first, torch.int32, dev)
        self.k = _intrinsics(k_matrix, B, dev)
        self.stream = _stream(dev)
        if not lsq:
            return
        nbytes = lib.prn_planes_ws_bytes(B, self.Ntot, H, W)
        if nbytes < 0:
            raise RuntimeError("prn_planes_ws_bytes: invalid sizes B=%d Ntot=%d H=%d W=%d" % (B, self.Ntot, H, W))
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.planes = torch.empty(self.Ntot, 4, dtype=torch.float64, device=dev)
        self.centroid = torch.empty(self.Ntot, 3, dtype=torch.float64, device=dev)
        self.valid = torch.empty(self.Ntot, dtype=torch.bool, device=dev)
        self.count = torch.empty(self.Ntot, dtype=torch.int64, device=dev)
        check(lib.prn_planes_fit(_p(self.depth), _p(self.ptrs), _p(self.first), _p(self.k), B, self.Ntot, H, W, _p(self.planes), _p(self.centroid),
                                 _p(self.valid), _p(self.count), _p(self.ws), self.stream), "prn_planes_fit")

    def render(self, depth_range=None):
        out = torch.empty_like(self.depth)
        lo, hi = (0.0, 0.0) if depth_range is None else (float(depth_range[0]), float(depth_range[1]))
        check(lib.prn_planes_render(_p(self.depth), _p(self.ptrs), _p(self.first), _p(self.k), _p(self.planes), _p(self.valid), self.B, self.Ntot,
                                    self.H, self.W, int(depth_range is not None), lo, hi, _p(out), _p(self.ws), self.stream), "prn_planes_render")
        return out

    def ransac(self, opts):
        """one prn_planes_ransac_fit call on the same inputs: planes, centroid and valid become the robust fit's (what render then paints),
        count the masks' pixel counts; adds inliers [Ntot] int64, hypothesis [Ntot] int32 and inlier_masks [Ntot,H,W] uint8"""
        B, H, W, dev = self.B, self.H, self.W, self.depth.device
        nbytes = lib.prn_planes_ransac_ws_bytes(B, self.Ntot, H, W, opts["hypotheses"])
        if nbytes < 0:
            raise RuntimeError("prn_planes_ransac_ws_bytes: invalid sizes B=%d Ntot=%d H=%d W=%d hypotheses=%d" % (B, self.Ntot, H, W, opts["hypotheses"]))
        self.ransac_ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.planes = torch.empty(self.Ntot, 4, dtype=torch.float64, device=dev)
        self.centroid = torch.empty(self.Ntot, 3, dtype=torch.float64, device=dev)
        self.valid = torch.empty(self.Ntot, dtype=torch.bool, device=dev)
        self.count = torch.empty(self.Ntot, dtype=torch.int64, device=dev)
        self.inliers = torch.empty(self.Ntot, dtype=torch.int64, device=dev)
        self.hypothesis = torch.empty(self.Ntot, dtype=torch.int32, device=dev)
        self.inlier_masks = torch.empty(self.Ntot, H, W, dtype=torch.uint8, device=dev)
        check(lib.prn_planes_ransac_fit(_p(self.depth), _p(self.ptrs), _p(self.first), _p(self.k), B, self.Ntot, H, W, opts["threshold"],
                                        int(opts["relative"]), opts["hypotheses"], opts["refine"], opts["seed"], _p(self.planes), _p(self.centroid),
                                        _p(self.valid), _p(self.count), _p(self.inliers), _p(self.hypothesis), _p(self.inlier_masks),
                                        _p(self.ransac_ws), self.stream), "prn_planes_ransac_fit")

    def split_inlier_masks(self):
        """per image, in the dtype of that image's masks"""
        parts = self.split(self.inlier_masks)
        return [p.view(torch.bool) if torch.is_tensor(m) and m.dtype == torch.bool else p for p, m in zip(parts, self.given)]

    def split(self, t):
        return list(torch.split(t, self.sizes))


def _robust_options(threshold=0.05, relative=False, hypotheses=256, refine=1, seed=0):
    """the checked keywords of fit_planes_ransac (ValueError outside the ranges of include/prn.h)"""
    import math
    import numbers
    for name, v, lo, hi in (("hypotheses", hypotheses, 1, 4096), ("refine", refine, 0, 8), ("seed", seed, 0, 2 ** 64 - 1)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (name, lo, hi, v))
    if isinstance(threshold, bool) or not isinstance(threshold, numbers.Real) or not (math.isfinite(threshold) and threshold > 0):
        raise ValueError("threshold must be a positive finite number, got %r" % (threshold,))
    return {"threshold": float(threshold), "relative": bool(relative), "hypotheses": int(hypotheses), "refine": int(refine), "seed": int(seed)}


@torch.no_grad()
def fit_planes(depth, masks, k_matrix):
    """Fits one plane per instance mask.

    depth    [B,1,H,W] fp32 device tensor (the predicted depth)
    masks    list of B [N_b,H,W] bool / uint8 device tensors (N_b may be 0; None = no instances)
    k_matrix intrinsics K, [3,3] or [B,3,3] (for an iBims-1 file: calib.T)
    -> (planes, valid, count): lists of B per-image tensors -- planes [N_b,4] fp64 (nx, ny, nz, d) in camera coordinates with
       n . X = d and d >= 0 (NaN rows for invalid instances), valid [N_b] bool, count [N_b] int64 (pixels of each mask)."""
    f = _Fit(depth, masks, k_matrix)
    return f.split(f.planes), f.split(f.valid), f.split(f.count)


@torch.no_grad()
def fit_planes_ransac(depth, masks, k_matrix, threshold=0.05, relative=False, hypotheses=256, refine=1, seed=0):
    """Fits one plane per instance mask robustly (csrc/prn_planes_ransac.hip): `hypotheses` three-point planes drawn
    from the mask (Philox4x32-10 keyed by `seed`, the hypothesis and the instance's index within its image), each scored by the mask pixels
    within `threshold` metres of it (relative=True: within threshold x the pixel's depth); the least-squares plane of the best hypothesis's
    inliers, then `refine` rounds of re-selecting the inliers of that plane and fitting them again.

    depth, masks, k_matrix as fit_planes.  hypotheses 1 .. 4096, refine 0 .. 8, threshold > 0 (ValueError otherwise).
    -> (planes, valid, count, inliers, hypothesis, inlier_masks): lists of B per-image tensors -- planes / valid as fit_planes (of the last
       inlier set), count [N_b] int64 (pixels of each MASK), inliers [N_b] int64 (pixels of the last inlier set), hypothesis [N_b] int32 (the
       chosen draw), inlier_masks [N_b,H,W] in the dtype of masks[b].  An invalid instance (no hypothesis with 3 inliers, or a degenerate
       inlier set) has a NaN plane, inliers 0, hypothesis -1 and an all-zero inlier mask.
    No host synchronisation; bit-identical run to run and between a batched call and per-image calls."""
    opts = _robust_options(threshold, relative, hypotheses, refine, seed)
    f = _Fit(depth, masks, k_matrix, lsq=False)
    f.ransac(opts)
    return f.split(f.planes), f.split(f.valid), f.split(f.count), f.split(f.inliers), f.split(f.hypothesis), f.split_inlier_masks()


@torch.no_grad()
def planar_depth(results, k_matrix, depth_range=None, clean=None, robust=None):
    """The planar depth of PlaneRecNet's eval-mode output (the list of per-image dicts): for every image a NEW dict with the
    input's entries plus
       pred_planes      [N,4] fp64 (see fit_planes; [0,4] when the image has no detections)
       pred_plane_valid [N] bool
       pred_plane_depth [1,1,H,W] fp32: pred_depth with every pixel a valid instance covers replaced by the plane depth of the
                        highest-index valid covering instance (the lowest-scored one: detections come in descending score order)
    depth_range = (lo, hi): values <= lo or >= hi become NaN afterwards (the iBims-1 exporter uses (0, 10)).
    clean = a dict of components.clean keywords (e.g. {"keep": "largest", "fill_holes": True}): every mask is cleaned on the device before the
    fit and the composition -- a speck on another surface tilts the least-squares plane of the whole instance -- and the dicts gain
       pred_plane_masks the masks that were used (pred_masks itself stays as it came)
    clean = None: the masks are used as they are.
    robust = a dict of fit_planes_ransac keywords (e.g. {"threshold": 0.05, "hypotheses": 256}; {} = its defaults): the planes come from the robust
    fit of the masks (after `clean`) -- a connected mask over two surfaces tilts the least-squares plane, cleaning does not help there.  The
    painted region is still the whole mask under the same owner rule (a valid instance owns its pixels whether or not they are inliers), and
    the dicts gain
       pred_plane_inliers      [N] int64 inlier pixels of each instance
       pred_plane_inlier_masks [N,H,W] the inliers, in the dtype of the masks
    robust = None: the least-squares fit.
    The input dicts and their tensors are not modified."""
    opts = None if robust is None else _robust_options(**robust)
    depth = torch.cat([r["pred_depth"].reshape(1, 1, *r["pred_depth"].shape[-2:]) for r in results]).float()
    masks = [r.get("pred_masks") for r in results]
    if clean is not None:
        from . import components
        masks = components.clean(masks, **clean)[0] if any(m is not None for m in masks) else masks
    f = _Fit(depth, masks, k_matrix)                             # (with robust too: its first pass leaves the owner map of the WHOLE masks)
    if opts is not None:
        f.ransac(opts)
        inliers, inlier_masks = f.split(f.inliers), f.split_inlier_masks()
    out = f.render(depth_range)
    planes, valid = f.split(f.planes), f.split(f.valid)
    new = []
    for b, r in enumerate(results):
        d = dict(r)
        d["pred_planes"], d["pred_plane_valid"], d["pred_plane_depth"] = planes[b], valid[b], out[b:b + 1]
        if opts is not None:
            d["pred_plane_inliers"], d["pred_plane_inlier_masks"] = inliers[b], inlier_masks[b]
        if clean is not None:
            d["pred_plane_masks"] = masks[b]
        new.append(d)
    return new
