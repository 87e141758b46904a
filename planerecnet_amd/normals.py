"""Surface normals of a depth map, their picture, and the angular error of two normal maps (include/prn.h: prn_normals, prn_normal_error;
DESIGN.md section 23).

`from_depth` turns (depth, K) into a unit normal per pixel where the depth is -- on the device -- under section 22's conventions:

  valid pixel  z finite and lo < z < hi in fp32 (depth_range, default (0, inf))
  point        P = (((double)u - cx) * z / fx, ((double)v - cy) * z / fy, z), fp64 in this order and NOT rounded to fp32
  usable q     a neighbour q of the centre c is usable iff it is inside the image and valid, carries c's label (labels given and same_label)
               and zmax - zmin <= max_gap * zmin (relative) or <= max_gap over the two depths, subtraction and product each rounded to fp32
  tangents     along u from E = (v, u+step) and W = (v, u-step): tu = P(E) - P(W) if both are usable, P(E) - P(c) or P(c) - P(W) if one is,
               else the pixel has no normal; along v the same from S = (v+step, u) and N = (v-step, u): tv = P(S) - P(N), ...
  normal       n = tv x tu (the orientation of section 22's triangles: a fronto-parallel surface gets (0,0,-1), n . P < 0), every product
               and difference rounded to fp64 on its own; L2 = (nx nx + ny ny) + nz nz; no normal unless L2 is finite and > 0; output
               n / sqrt(L2) per component, negated with sign="plane" (fit_planes' n . X = d >= 0), each rounded to fp32 once
  no normal    (0,0,0), valid False

The outputs are once-rounded fp64 expressions, so they are specified bit for bit.  Device tensors run on the device (one launch whatever
the batch, no host synchronisation, inputs untouched), CPU tensors on the host in numpy with the same outputs bit for bit.
"""
import ctypes
import math
import numbers

import numpy as np
import torch

from ._masks import _bytes_buffer, _describe, _p, _stream
from .reconstruct import _check_inputs, _intrinsics_np

__all__ = ["from_depth", "colorize", "angular_error", "error_stats", "NormalErrorAccumulator", "from_planes", "block_pixels", "error_bins", "MAX_THRESHOLDS"]

RELATIVE, SAME_LABEL, PLANE_SIGN = 1, 2, 4         # include/prn.h: PRN_NORMALS_*
MAX_THRESHOLDS = 8                                 # PRN_NORMAL_ERROR_MAX_T
_BINS = 4096                                       # prn_normal_error_bins() (the host path needs no library)
_MAX_BATCH = 65535


def block_pixels():
    """consecutive pixels one workgroup of the device path takes (prn_normals_block_pixels)"""
    from ._lib import lib
    return int(lib.prn_normals_block_pixels())


def error_bins():
    """chord bins of the error histogram (prn_normal_error_bins)"""
    return _BINS


def _sign(sign, what):
    if sign not in ("camera", "plane"):
        raise ValueError("%s: sign must be \"camera\" (n . P < 0) or \"plane\" (n . X = d >= 0), got %r" % (what, sign))
    return sign == "plane"


# ---- host path (numpy) -----------------------------------------------------------------------------------------------------------

def _shift(a, dv, du, fill):
    """out[v, u] = a[v + dv, u + du] where that lies inside, else fill"""
    H, W = a.shape[:2]
    out = np.full(a.shape, fill, a.dtype)
    if abs(dv) < H and abs(du) < W:
        out[max(0, -dv):H - max(0, dv), max(0, -du):W - max(0, du)] = a[max(0, dv):H + min(0, dv), max(0, du):W + min(0, du)]
    return out


def _normals_np(z, lab, k, step, lo, hi, gap, relative, same_label, plane_sign):
    """one image: z [H,W] float32, lab [H,W] int32 or None, k [9] float64 -> (normals [H,W,3] float32, valid [H,W] bool)"""
    H, W = z.shape
    with np.errstate(all="ignore"):
        ok = np.isfinite(z) & (z > lo) & (z < hi)
        v, u = np.mgrid[:H, :W]
        z64 = z.astype(np.float64)
        P = np.stack([(u.astype(np.float64) - k[2]) * z64 / k[0], (v.astype(np.float64) - k[5]) * z64 / k[4], z64], -1)

        def neighbour(dv, du):
            zq = _shift(z, dv, du, np.float32(np.nan))
            use = ok & _shift(ok, dv, du, False)
            if lab is not None and same_label:
                use &= _shift(lab, dv, du, 0) == lab
            zmin = np.minimum(z, zq)
            use &= (np.maximum(z, zq) - zmin) <= (gap * zmin if relative else gap)
            return use, _shift(P, dv, du, 0.0)

        def tangent(plus, minus):
            (up, pp), (um, pm) = plus, minus
            return np.where(up[..., None], pp, P) - np.where(um[..., None], pm, P), up | um

        tu, has_u = tangent(neighbour(0, step), neighbour(0, -step))
        tv, has_v = tangent(neighbour(step, 0), neighbour(-step, 0))
        raw = np.stack([tv[..., 1] * tu[..., 2] - tv[..., 2] * tu[..., 1], tv[..., 2] * tu[..., 0] - tv[..., 0] * tu[..., 2],
                        tv[..., 0] * tu[..., 1] - tv[..., 1] * tu[..., 0]], -1)
        l2 = (raw[..., 0] * raw[..., 0] + raw[..., 1] * raw[..., 1]) + raw[..., 2] * raw[..., 2]
        valid = ok & has_u & has_v & np.isfinite(l2) & (l2 > 0)
        n = (raw / np.sqrt(l2)[..., None]).astype(np.float32)
        if plane_sign:
            n = -n
        n[~valid] = 0.0
    return n, valid


def _bytes_np(n, valid):
    """normals [...,3] float32, valid [...] bool -> the picture's bytes [...,3] (BGR = z, y, x)"""
    with np.errstate(all="ignore"):
        b = np.rint((n[..., ::-1].astype(np.float64) * 0.5 + 0.5) * 255.0)
    return np.where(valid[..., None], b, 0.0).astype(np.uint8)


# ---- from_depth --------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def from_depth(depth, k_matrix, labels=None, step=1, max_gap=0.05, relative=True, same_label=True, depth_range=(0.0, math.inf), sign="camera", image=False):
    """The normal map of a depth map (module docstring for the rules).

    depth        [H,W], [1,H,W] or [B,1,H,W] fp32; H * W < 2^24
    k_matrix     intrinsics K, [3,3] or [B,3,3] (tensor anywhere, or an array)
    labels       int32 [H,W] or [B,H,W] on depth's device (plane_eval.label_map's output) or None
    step         the neighbours' distance in pixels, >= 1
    max_gap      the largest depth spread of a pixel and a neighbour it uses: a fraction of the smaller depth (relative) or metres
    same_label   with labels: a pixel uses only neighbours of its own label
    sign         "camera": n . P < 0 (the normal faces the camera); "plane": negated, fit_planes' convention
    image        True: also the picture, uint8 [B,H,W,3] BGR (channel 0 = z, 1 = y, 2 = x; byte = rint((n * 0.5 + 0.5) * 255), ties to even)
    -> (normals [B,H,W,3] fp32, valid [B,H,W] bool, image or None) on depth's device; pixels without a normal hold zeros."""
    what = "normals.from_depth"
    B, H, W, lo, hi, gap = _check_inputs(depth, labels, None, depth_range, max_gap, what)
    if isinstance(step, bool) or not isinstance(step, numbers.Integral) or not 1 <= int(step) < 2 ** 31:
        raise ValueError("%s: step must be an integer >= 1, got %r" % (what, step))
    step, plane = int(step), _sign(sign, what)
    dev = depth.device
    z = depth.detach().reshape(B, H, W).contiguous()
    lab = None if labels is None else labels.reshape(B, H, W).contiguous()
    if not z.is_cuda:
        if dev.type != "cpu":
            raise RuntimeError("%s: depth must be a device or a CPU tensor, got %s" % (what, _describe(depth)))
        k = _intrinsics_np(k_matrix, B)
        n, ok = np.zeros((B, H, W, 3), np.float32), np.zeros((B, H, W), bool)
        for b in range(B):
            n[b], ok[b] = _normals_np(z[b].numpy(), None if lab is None else lab[b].numpy(), k[b], step, lo, hi, gap, relative, same_label, plane)
        return torch.from_numpy(n), torch.from_numpy(ok), torch.from_numpy(_bytes_np(n, ok)) if image else None
    from ._lib import check, lib
    from .planes import _intrinsics
    k = _intrinsics(k_matrix, B, dev)
    n = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
    ok = _bytes_buffer(B * H * W, dev).view(B, H, W)
    img = _bytes_buffer(B * H * W * 3, dev).view(B, H, W, 3) if image else None
    flags = (RELATIVE if relative else 0) | (SAME_LABEL if same_label else 0) | (PLANE_SIGN if plane else 0)
    stream = _stream(dev)
    for b0 in range(0, B, _MAX_BATCH):
        nb = min(B, b0 + _MAX_BATCH) - b0
        check(lib.prn_normals(_p(z[b0:]), None if lab is None else _p(lab[b0:]), _p(k[b0:]), nb, H, W, step, float(lo), float(hi), float(gap), flags,
                              _p(n[b0:]), _p(ok[b0:]), None if img is None else _p(img[b0:]), stream), "prn_normals")
    return n, ok.view(torch.bool), img


def colorize(normals, valid):
    """The picture from_depth(image=True) returns, from a normal map and its validity in torch (any device) or numpy: uint8 [...,3] BGR with
    channel 0 = z, 1 = y, 2 = x, byte = rint(((double)n * 0.5 + 0.5) * 255), ties to even; (0,0,0) where valid is False."""
    if torch.is_tensor(normals):
        b = torch.round((normals.flip(-1).double() * 0.5 + 0.5) * 255.0)
        return torch.where(torch.as_tensor(valid, device=normals.device).bool()[..., None], b, torch.zeros_like(b)).to(torch.uint8)
    return _bytes_np(np.asarray(normals, dtype=np.float32), np.asarray(valid).astype(bool))


# ---- angular error ---------------------------------------------------------------------------------------------------------------

def _thr2(thresholds, what):
    t = [float(x) for x in thresholds]
    if len(t) > MAX_THRESHOLDS or any(not 0.0 <= x <= 180.0 for x in t):
        raise ValueError("%s: at most %d thresholds, in degrees in [0, 180]; got %r" % (what, MAX_THRESHOLDS, thresholds))
    return [(2.0 * math.sin(math.radians(x) / 2.0)) ** 2 for x in t]


def _pairs(a, va, b, vb, what):
    """-> (B, n, a [B,n,3] fp32, va [B,n] bytes, b, vb), contiguous"""
    if not (torch.is_tensor(a) and a.dtype == torch.float32 and a.dim() in (2, 3, 4) and a.shape[-1] == 3 and a.numel() > 0):
        raise RuntimeError("%s: a must be a non-empty fp32 [n,3], [H,W,3] or [B,H,W,3] tensor, got %s" % (what, _describe(a)))
    if not (torch.is_tensor(b) and b.dtype == torch.float32 and b.shape == a.shape and b.device == a.device):
        raise RuntimeError("%s: b must match a (%s), got %s" % (what, _describe(a), _describe(b)))
    B = int(a.shape[0]) if a.dim() == 4 else 1
    n = a.numel() // (3 * B)
    out = [a.detach().reshape(B, n, 3).contiguous(), None, b.detach().reshape(B, n, 3).contiguous(), None]
    for i, v in ((1, va), (3, vb)):
        if not (torch.is_tensor(v) and v.dtype in (torch.bool, torch.uint8) and v.shape == a.shape[:-1] and v.device == a.device):
            raise RuntimeError("%s: a validity map must be a bool / uint8 tensor of a's shape without its last axis on a's device, got %s" % (what, _describe(v)))
        v = v.reshape(B, n).contiguous()
        out[i] = v.view(torch.uint8) if v.dtype == torch.bool else v
    return (B, n) + tuple(out)


def _error_np(a, va, b, vb, thr2):
    """one image pair: a, b [n,3] float32, va, vb [n] -> (hist [BINS], within [T], count) int64"""
    both = (va != 0) & (vb != 0)
    with np.errstate(all="ignore"):
        d = a[both].astype(np.float64) - b[both].astype(np.float64)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        t = np.floor(np.sqrt(d2) * (_BINS // 2))
        bins = np.where(t < _BINS - 1, t, _BINS - 1).astype(np.int64)                    # (a NaN chord: the last bin)
    return (np.bincount(bins, minlength=_BINS).astype(np.int64), np.array([int((d2 <= x).sum()) for x in thr2], dtype=np.int64).reshape(len(thr2)),
            np.int64(d2.shape[0]))


def _error_into(B, n, a, va, b, vb, thr2, hist, within, count):
    """adds the tables of B pairs of n pixels into device int64 hist [B,BINS], within [B,T], count [B] (no synchronisation)"""
    from ._lib import check, lib
    arr = (ctypes.c_double * max(1, len(thr2)))(*thr2)
    check(lib.prn_normal_error(_p(a), _p(va), _p(b), _p(vb), B, n, arr, len(thr2), _p(hist), _p(within) if len(thr2) else None, _p(count), _stream(a.device)),
          "prn_normal_error")


@torch.no_grad()
def angular_error(a, va, b, vb, thresholds=(11.25, 22.5, 30)):
    """The angle between two unit normal maps over the pixels valid in both, as counts (integers: exact and identical run to run).

    a, b         fp32 [B,H,W,3], [H,W,3] or [n,3] (B = 1) on one device; va, vb: their bool / uint8 validity, a's shape without the 3
    thresholds   at most 8 angles in degrees in [0, 180]; compared as squared chords, thr2 = (2 sin(t / 2))^2 in fp64
    Per pixel d = (double)a - (double)b, d2 = (dx dx + dy dy) + dz dz, chord = sqrt(d2) = 2 sin(angle / 2),
    bin = min(BINS - 1, floor(chord * (BINS / 2))), BINS = error_bins() = 4096.
    -> (hist [B,BINS], within [B,T], count [B]) int64 on a's device: `error_stats` turns them into mean / median / RMSE / shares."""
    what = "normals.angular_error"
    thr2 = _thr2(thresholds, what)
    B, n, a, va, b, vb = _pairs(a, va, b, vb, what)
    if not a.is_cuda:
        parts = [_error_np(a[i].numpy(), va[i].numpy(), b[i].numpy(), vb[i].numpy(), thr2) for i in range(B)]
        return tuple(torch.from_numpy(np.stack([p[j] for p in parts])) for j in range(3))
    if B > _MAX_BATCH or n >= 2 ** 31:
        raise RuntimeError("%s: at most %d images of fewer than 2^31 pixels, got %d x %d" % (what, _MAX_BATCH, B, n))
    dev = a.device
    hist, within, count = (torch.zeros(B, s, dtype=torch.int64, device=dev) for s in (_BINS, len(thr2), 1))
    _error_into(B, n, a, va, b, vb, thr2, hist, within, count)
    return hist, within, count.reshape(B)


def error_stats(hist, within, count):
    """Host, fp64: the pooled statistics of angular_error's tables (tensors or arrays; a leading batch axis is summed).

    A bin's angle is that of its centre chord: c_i = (i + 0.5) * 2 / BINS, theta_i = degrees(2 asin(min(1, c_i / 2))).  mean = sum h theta / n,
    rmse = sqrt(sum h theta^2 / n), median = theta_i of the first bin whose cumulative count reaches (n + 1) // 2, shares = within / n; all NaN
    at n = 0.  A bin is 0.028 degrees wide at 0 degrees and 0.040 at 90 (wider towards 180, where the chord flattens): mean and median are
    right to within half the widest occupied bin, the shares are exact.
    -> {"mean", "median", "rmse": floats in degrees, "within": float64 [T] shares, "count": int}"""
    h = np.asarray(hist.cpu() if torch.is_tensor(hist) else hist, dtype=np.int64).reshape(-1, _BINS).sum(0)
    w = np.asarray(within.cpu() if torch.is_tensor(within) else within, dtype=np.int64)
    w = w.reshape(-1, w.shape[-1]).sum(0) if w.ndim else w.reshape(1)
    n = int(np.asarray(count.cpu() if torch.is_tensor(count) else count, dtype=np.int64).sum())
    if n == 0:
        return {"mean": math.nan, "median": math.nan, "rmse": math.nan, "within": np.full(w.shape, np.nan), "count": 0}
    theta = bin_angles()
    hf = h.astype(np.float64)
    median = theta[int(np.searchsorted(np.cumsum(h), (n + 1) // 2, side="left"))]
    return {"mean": float((hf * theta).sum() / n), "median": float(median), "rmse": float(math.sqrt((hf * theta * theta).sum() / n)),
            "within": w.astype(np.float64) / n, "count": n}


def bin_angles():
    """theta_i in degrees of every histogram bin's centre chord, float64 [BINS]"""
    c = (np.arange(_BINS, dtype=np.float64) + 0.5) * 2.0 / _BINS
    return np.degrees(2.0 * np.arcsin(np.minimum(1.0, c / 2.0)))


class NormalErrorAccumulator:
    """A run's pooled error tables, kept where the maps are: add() adds a batch of map pairs (every image's pixels into one table; no host
    synchronisation on a device), result() downloads once and returns error_stats' dict."""

    def __init__(self, thresholds=(11.25, 22.5, 30), device="cpu"):
        self.thresholds = tuple(float(t) for t in thresholds)
        self._thr2 = _thr2(self.thresholds, "NormalErrorAccumulator")
        self.device = torch.zeros(0, device=device).device          # ("cuda" -> the current device, with its index)
        self._tables = torch.zeros(_BINS + len(self._thr2) + 1, dtype=torch.int64, device=self.device)    # hist | within | count

    def add(self, a, va, b, vb):
        what = "NormalErrorAccumulator.add"
        B, n, a, va, b, vb = _pairs(a, va, b, vb, what)
        if a.device != self.device:
            raise RuntimeError("%s: the maps are on %s, the accumulator on %s" % (what, a.device, self.device))
        T = len(self._thr2)
        if not a.is_cuda:
            h, w, c = _error_np(a.reshape(-1, 3).numpy(), va.reshape(-1).numpy(), b.reshape(-1, 3).numpy(), vb.reshape(-1).numpy(), self._thr2)
            self._tables += torch.from_numpy(np.concatenate([h, w, c.reshape(1)]))
            return self
        if B * n >= 2 ** 31:
            raise RuntimeError("%s: fewer than 2^31 pixels a call, got %d x %d" % (what, B, n))
        t = self._tables
        _error_into(1, B * n, a, va, b, vb, self._thr2, t[:_BINS], t[_BINS:_BINS + T], t[_BINS + T:])   # the images lie back to back: one image of B n pixels
        return self

    def tables(self):
        """-> (hist [BINS], within [T], count) as int64 numpy arrays: one download"""
        t = self._tables.cpu().numpy()
        T = len(self._thr2)
        return t[:_BINS].copy(), t[_BINS:_BINS + T].copy(), t[_BINS + T]

    def result(self):
        return error_stats(*self.tables())


# ---- from planes -----------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def from_planes(labels, planes, sign="camera"):
    """Paints each label's plane normal: labels int [H,W] (plane_eval.label_map's owner map: 0 = no plane, i = planes[i - 1]), planes [N,>=3]
    (fit_planes' rows (nx, ny, nz, d) with n . X = d >= 0; NaN rows for planes that were not fitted).  sign="camera" negates them (n . P < 0,
    from_depth's default), "plane" keeps them.  Plain indexing on labels' device, no kernel and no synchronisation.
    -> (normals [H,W,3] fp32, valid [H,W] bool); label 0, labels past N and NaN planes give invalid pixels holding zeros."""
    plane = _sign(sign, "normals.from_planes")
    if not (torch.is_tensor(labels) and labels.dim() == 2 and not labels.dtype.is_floating_point):
        raise RuntimeError("normals.from_planes: labels must be an integer [H,W] tensor, got %s" % _describe(labels))
    planes = torch.as_tensor(planes).to(labels.device)
    if planes.dim() != 2 or planes.shape[1] < 3:
        raise RuntimeError("normals.from_planes: planes must be [N,>=3], got %s" % _describe(planes))
    N = int(planes.shape[0])
    n = planes[:, :3].to(torch.float32)
    table = torch.cat([torch.full((1, 3), math.nan, dtype=torch.float32, device=labels.device), n if plane else -n])
    idx = labels.long()
    picked = table[torch.where((idx >= 1) & (idx <= N), idx, torch.zeros_like(idx))]
    valid = torch.isfinite(picked).all(-1)
    return torch.where(valid[..., None], picked, torch.zeros_like(picked)), valid
