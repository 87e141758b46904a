"""Erosion, dilation and the inner boundary band of instance masks (include/prn.h: prn_morph).

PlaneRecNet's depth-gradient loss exists to put mask edges on depth discontinuities, and mask IoU hardly sees an edge: Boundary IoU (Cheng et
al., CVPR 2021; metrics.boundary_iou) compares the bands `boundary` returns.  The one primitive underneath is binary erosion of a ragged
batch of masks where they already are -- on the device.  All of it is integer-exact and defined to coincide with scipy.ndimage:

  erode(m, r, border)   a pixel is set iff every pixel of the (2r+1) x (2r+1) square round it is set, pixels outside the image having the
                        value `border` -- binary_erosion(m, ones((3, 3)), iterations=r, border_value=border).  r = 0 copies; r >= max(H, W)
                        is legal.
  dilate(m, r, border)  set iff any pixel of the square is set -- binary_dilation(...), and ~erode(~m, r, 1 - border).
  boundary(m, r)        m & ~erode(m, r, border=0): the inner band.  The image edge counts as background (the published definition pads the
                        mask with zeros), so a mask clipped by the frame has a band along the frame; a non-empty mask has a non-empty band
                        for r >= 1; r = 0 gives an empty band.
  boundary_radius       max(1, round(ratio * image diagonal)): 16 at 480 x 640, 24 at 736 x 960 with the metric's ratio 0.02.

Device tensors run on the device (three launches per chunk, no host synchronisation, inputs untouched), CPU tensors on the host in numpy (no
scipy), with the same outputs bit for bit -- the rule of components.clean.
"""
import ctypes
import math

import numpy as np
import torch

from ._masks import _as_bytes, _bytes_buffer, _inputs, _p, _split, _stream, ragged_chunks

__all__ = ["erode", "dilate", "boundary", "boundary_radius", "TILE_ROWS", "TILE_WORDS", "LDS_RADIUS"]

TILE_ROWS, TILE_WORDS = 64, 4      # rows x 64-bit words of the tile one workgroup of the column pass owns (include/prn.h: PRN_MORPH_TILE_ROWS / _WORDS)
LDS_RADIUS = 32                    # up to this min(radius, H) the column pass works in LDS, beyond it from the workspace (PRN_MORPH_LDS_RADIUS)
ERODE, DILATE, BOUNDARY = 0, 1, 2


def boundary_radius(H, W, ratio=0.02):
    """The band width of Boundary IoU for an H x W image: `ratio` of the diagonal, at least one pixel."""
    return max(1, int(round(ratio * math.sqrt(H * H + W * W))))


def _check(radius, border, what, shape):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or radius < 0:
        raise ValueError("%s: radius must be an integer >= 0, got %r (masks %s)" % (what, radius, shape))
    if isinstance(border, bool) or border not in (0, 1):
        raise ValueError("%s: border must be 0 or 1, got %r (masks %s)" % (what, border, shape))
    return int(min(radius, 2 ** 31 - 1)), int(border)


# ---- host path (numpy) -----------------------------------------------------------------------------------------------------------

def _window_and(a, n, axis):
    """AND over every window of n consecutive entries along `axis` (the axis shrinks by n - 1): doubling, then one overlapping step"""
    def cut(v, lo, hi):
        idx = [slice(None)] * v.ndim
        idx[axis] = slice(lo, hi)
        return v[tuple(idx)]
    L = 1
    while 2 * L <= n:
        a = cut(a, 0, a.shape[axis] - L) & cut(a, L, None)
        L *= 2
    if L < n:
        a = cut(a, 0, a.shape[axis] - (n - L)) & cut(a, n - L, None)
    return a


def _erode_np(m, radius, border):
    """m [N,H,W] bool"""
    for axis in (2, 1):
        r = min(radius, m.shape[axis])               # (a window that long already covers the axis and both borders)
        pad = [(0, 0)] * 3
        pad[axis] = (r, r)
        m = _window_and(np.pad(m, pad, constant_values=bool(border)), 2 * r + 1, axis)
    return m


def _morph_np(m, op, radius, border):
    if op == ERODE:
        return _erode_np(m, radius, border)
    if op == DILATE:
        return ~_erode_np(~m, radius, 1 - border)
    return m & ~_erode_np(m, radius, 0)


# ---- device path -----------------------------------------------------------------------------------------------------------------

def _device_run(parts, op, radius, border, out, area, max_workspace_bytes, what):
    """parts: contiguous uint8 [N_b,H,W] device tensors with N_b > 0, walked in chunks whose workspace stays under the limit"""
    from ._lib import check, lib
    dev = parts[0].device
    H, W = int(parts[0].shape[1]), int(parts[0].shape[2])
    per_mask = lib.prn_morph_ws_bytes(1, H, W, radius)
    if per_mask < 0:
        raise RuntimeError("%s: H * W must be below 2^31, got %d x %d" % (what, H, W))
    for g0, g1, ptrs, first in ragged_chunks(parts, per_mask, max_workspace_bytes):
        ws = torch.empty((lib.prn_morph_ws_bytes(g1 - g0, H, W, radius) + 7) // 8 * 2, dtype=torch.int32, device=dev)
        check(lib.prn_morph(_p(ptrs), _p(first), ptrs.numel(), g1 - g0, H, W, op, radius, border, ctypes.c_void_p(out.data_ptr() + g0 * H * W),
                            ctypes.c_void_p(area.data_ptr() + 4 * g0), _p(ws), _stream(dev)), "prn_morph")
        del ptrs, first, ws                                          # (stream-ordered allocator: reuse after this point is ordered behind the launches)


@torch.no_grad()
def _morph(masks, op, radius, border, what, max_workspace_bytes, return_area):
    is_list, parts, ref = _inputs(masks, what)
    radius, border = _check(radius, border, what, "none" if ref is None else tuple(ref.shape))
    sizes = [0 if m is None else int(m.shape[0]) for m in parts]
    if ref is None:
        out, area = [None] * len(parts), [torch.zeros(0, dtype=torch.int32) for _ in parts]
        return (out, area) if return_area else out
    H, W = int(ref.shape[1]), int(ref.shape[2])
    Ntot, dev = sum(sizes), ref.device
    if not ref.is_cuda:
        m = np.concatenate([p.numpy().astype(bool) for p in parts if p is not None]) if Ntot else np.zeros((0, H, W), bool)
        o = _morph_np(m, op, radius, border) if Ntot and H * W else np.zeros((Ntot, H, W), bool)
        out = torch.from_numpy(np.ascontiguousarray(o)).to(ref.dtype)
        area = torch.from_numpy(o.reshape(Ntot, H * W).sum(1).astype(np.int32))
    else:
        out = _bytes_buffer(Ntot * H * W, dev).view(Ntot, H, W)
        area = torch.empty(Ntot, dtype=torch.int32, device=dev)
        live = [_as_bytes(p) for p in parts if p is not None and p.shape[0]]
        if Ntot and H * W:
            _device_run(live, op, radius, border, out, area, max_workspace_bytes, what)
        elif Ntot:
            area.zero_()
        if ref.dtype == torch.bool:
            out = out.view(torch.bool)
    if is_list:
        empty = torch.zeros(0, dtype=torch.int32, device=dev)
        out = _split(out, sizes, parts, True)
        area = [a if a is not None else empty for a in _split(area, sizes, parts, True)]
    return (out, area) if return_area else out


def erode(masks, radius, border=0, max_workspace_bytes=256 << 20, return_area=False):
    """Binary erosion by the (2 radius + 1)^2 square; pixels outside the image have the value `border`.

    masks   [N,H,W] bool / uint8 tensor (non-zero = set), or a list of per-image tensors (None or N_b = 0: no instances)
    -> the eroded masks in the input's dtype and shape (set = 1); a list gives a list (None where the input had None).  With return_area
       also the int32 [N] number of set pixels of every output mask.  On the device the masks are walked in chunks whose workspace (two
       bits per pixel per mask in flight, rows rounded up to 64 pixels) stays under max_workspace_bytes; nothing is read back."""
    return _morph(masks, ERODE, radius, border, "erode", max_workspace_bytes, return_area)


def dilate(masks, radius, border=0, max_workspace_bytes=256 << 20, return_area=False):
    """Binary dilation by the (2 radius + 1)^2 square (= ~erode(~masks, radius, 1 - border)); arguments and result as for `erode`."""
    return _morph(masks, DILATE, radius, border, "dilate", max_workspace_bytes, return_area)


def boundary(masks, radius, max_workspace_bytes=256 << 20, return_area=False):
    """The inner boundary band masks & ~erode(masks, radius, border=0) of Boundary IoU; arguments and result as for `erode`."""
    return _morph(masks, BOUNDARY, radius, 0, "boundary", max_workspace_bytes, return_area)
