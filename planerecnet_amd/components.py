"""Connected components of instance masks: labels, and masks cleaned to one region (include/prn.h: prn_ccl_*).

Everything downstream of the detector treats an instance mask as one planar surface, but a SOLO mask is a thresholded, resized map: it has
specks on other surfaces, fragments split by an occluder and pin-holes.  `label` numbers the components of every mask, `clean` keeps the
largest (or every large enough) component and optionally fills the holes of what it kept, `clean_results` applies that to the network's
eval-mode output.  All of it is integer-exact and defined to coincide with scipy.ndimage:

  label   components are numbered 1..K in ascending order of their smallest row-major index y * W + x -- ndimage.label with
          structure=ones((3, 3)) for connectivity 8 (the default), the cross for 4
  clean   per mask: (1) label it, take every component's area; (2) keep="largest": the component of maximal area, on a tie the lowest label,
          nothing if its area < min_area; keep="all": every component with area >= min_area; (3) fill_holes: in the mask selected by (2),
          every unset pixel becomes set unless unset pixels connect it to an unset pixel on the image border under the dual connectivity
          (4 for a foreground of 8 and the reverse) -- ndimage.binary_fill_holes with the cross / the full structure.  No mask is dropped:
          one that loses everything comes back empty.

Device tensors run on the device (a ragged batch in five to ten launches per chunk, no host synchronisation, inputs untouched), CPU tensors
on the host in numpy (no scipy), with the same outputs bit for bit -- the rule of nms.mask_nms.
"""
import ctypes

import numpy as np
import torch

from ._masks import _as_bytes, _bytes_buffer, _inputs, _p, _split, _stream, ragged_chunks

__all__ = ["label", "clean", "clean_results", "TILE"]

TILE = (32, 64)          # rows x columns of the tile one workgroup labels in LDS (include/prn.h: PRN_CCL_TILE_H / PRN_CCL_TILE_W)


def _check_connectivity(connectivity, what):
    if connectivity not in (4, 8):
        raise RuntimeError("%s: connectivity must be 4 or 8, got %r" % (what, connectivity))
    return int(connectivity)


# ---- host path (numpy) -----------------------------------------------------------------------------------------------------------

_OFFSETS = {4: ((-1, 0), (1, 0), (0, -1), (0, 1)), 8: ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))}


def _roots_np(m, connectivity):
    """m [N,H,W] bool -> [N,H,W] int64: the smallest row-major index of every set pixel's component (H*W on unset pixels).  Minimum
    propagation over the neighbours with pointer jumping (a label is always the index of a pixel of the same component)."""
    N, H, W = m.shape
    HW = H * W
    big = HW
    lab = np.where(m, np.arange(HW, dtype=np.int64).reshape(1, H, W), big)
    active = np.arange(N)                                            # masks that changed in the last round
    while active.size:
        A = active.size
        cur, set_ = lab[active], m[active]
        new = cur.copy()
        for dy, dx in _OFFSETS[connectivity]:
            ys, yd = (slice(0, H - 1), slice(1, H)) if dy == -1 else ((slice(1, H), slice(0, H - 1)) if dy == 1 else (slice(None), slice(None)))
            xs, xd = (slice(0, W - 1), slice(1, W)) if dx == -1 else ((slice(1, W), slice(0, W - 1)) if dx == 1 else (slice(None), slice(None)))
            np.minimum(new[:, yd, xd], cur[:, ys, xs], out=new[:, yd, xd])
        new = np.where(set_, new, big)
        base = (np.arange(A, dtype=np.int64) * (HW + 1)).reshape(A, 1, 1)
        while True:                                                  # new <- new[new] until it is stable: every chain collapses onto its end
            table = np.concatenate([new.reshape(A, HW), np.full((A, 1), big, np.int64)], 1).reshape(-1)
            nxt = table[new + base]
            if np.array_equal(nxt, new):
                break
            new = nxt
        changed = (new != cur).reshape(A, -1).any(1)
        lab[active] = new
        active = active[changed]
    return lab


def _label_np(m, connectivity):
    """-> (labels int32 [N,H,W], count int32 [N], roots): labels 1..K by ascending first pixel"""
    N, H, W = m.shape
    roots = _roots_np(m, connectivity)
    labels = np.zeros((N, H, W), np.int32)
    count = np.zeros(N, np.int32)
    for n in range(N):
        r = np.unique(roots[n][m[n]])
        count[n] = r.size
        if r.size:
            labels[n][m[n]] = (np.searchsorted(r, roots[n][m[n]]) + 1).astype(np.int32)
    return labels, count


def _clean_np(m, connectivity, keep, min_area, fill_holes):
    N, H, W = m.shape
    labels, count = _label_np(m, connectivity)
    out = np.zeros((N, H, W), bool)
    kept, largest, area = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
    for n in range(N):
        areas = np.bincount(labels[n].reshape(-1), minlength=int(count[n]) + 1)[1:]
        if areas.size == 0:
            continue
        largest[n] = areas.max()
        if keep == "largest":
            chosen = np.array([int(np.argmax(areas)) + 1]) if areas.max() >= min_area else np.zeros(0, np.int64)      # (argmax: the first maximum)
        else:
            chosen = np.flatnonzero(areas >= min_area) + 1
        kept[n] = chosen.size
        out[n] = np.isin(labels[n], chosen)
    if fill_holes and N:
        back, _ = _label_np(~out, 4 if connectivity == 8 else 8)
        for n in range(N):
            b = back[n]
            outside = np.unique(np.concatenate([b[0], b[-1], b[:, 0], b[:, -1]]))
            out[n] |= ~np.isin(b, outside[outside > 0]) & (b > 0)
    area[:] = out.reshape(N, -1).sum(1)
    return out, {"count": count, "kept": kept, "largest": largest, "area": area}


# ---- device path -----------------------------------------------------------------------------------------------------------------

def _device_run(parts, what, max_workspace_bytes, call):
    """parts: contiguous uint8 [N_b,H,W] device tensors with N_b > 0.  call(lib, ptrs_dev, first_dev, B, n, H, W, g0, ws, stream) per chunk."""
    from ._lib import lib
    dev = parts[0].device
    H, W = int(parts[0].shape[1]), int(parts[0].shape[2])
    per_mask = lib.prn_ccl_ws_bytes(1, H, W)
    if per_mask < 0:
        raise RuntimeError("%s: H * W must be below 2^31, got %d x %d" % (what, H, W))
    for g0, g1, ptrs, first in ragged_chunks(parts, per_mask, max_workspace_bytes):
        ws = torch.empty((lib.prn_ccl_ws_bytes(g1 - g0, H, W) + 7) // 8 * 2, dtype=torch.int32, device=dev)
        call(lib, ptrs, first, ptrs.numel(), g1 - g0, H, W, g0, ws, _stream(dev))
        del ptrs, first, ws                                          # (stream-ordered allocator: reuse after this point is ordered behind the launches)


@torch.no_grad()
def label(masks, connectivity=8):
    """Connected components of every mask.

    masks   [N,H,W] bool / uint8 tensor (non-zero = set), or a list of per-image tensors (None or N_b = 0: no instances)
    -> (labels, count): labels int32 [N,H,W], 0 on unset pixels and 1..K on the components in ascending order of their first pixel in
       row-major order; count int32 [N] = K.  A list gives lists (None where the input had None; count is then an empty tensor)."""
    connectivity = _check_connectivity(connectivity, "label")
    is_list, parts, ref = _inputs(masks, "label")
    sizes = [0 if m is None else int(m.shape[0]) for m in parts]
    if ref is None:
        return [None] * len(parts), [torch.zeros(0, dtype=torch.int32) for _ in parts]
    H, W = int(ref.shape[1]), int(ref.shape[2])
    Ntot, dev = sum(sizes), ref.device
    if not ref.is_cuda:
        m = np.concatenate([p.numpy().astype(bool) for p in parts if p is not None]) if Ntot else np.zeros((0, H, W), bool)
        lab, cnt = _label_np(m, connectivity) if Ntot and H * W else (np.zeros((Ntot, H, W), np.int32), np.zeros(Ntot, np.int32))
        labels, count = torch.from_numpy(lab), torch.from_numpy(cnt)
    else:
        labels = torch.empty(Ntot, H, W, dtype=torch.int32, device=dev)
        count = torch.empty(Ntot, dtype=torch.int32, device=dev)
        live = [_as_bytes(p) for p in parts if p is not None and p.shape[0]]
        if Ntot and H * W:
            from ._lib import check

            def call(lib, ptrs, first, B, n, H, W, g0, ws, stream):
                check(lib.prn_ccl_label(_p(ptrs), _p(first), B, n, H, W, connectivity, _p(labels[g0:]) if g0 else _p(labels),
                                        ctypes.c_void_p(count.data_ptr() + 4 * g0), _p(ws), stream), "prn_ccl_label")
            _device_run(live, "label", 256 << 20, call)
    if not is_list:
        return labels, count
    return _split(labels, sizes, parts, True), [c if c is not None else torch.zeros(0, dtype=torch.int32, device=dev) for c in _split(count, sizes, parts, True)]


@torch.no_grad()
def clean(masks, connectivity=8, keep="largest", min_area=0, fill_holes=False, max_workspace_bytes=256 << 20):
    """Every mask reduced to its largest component (keep="largest"; a tie: the first in row-major order) or to its components of at least
    min_area pixels (keep="all"), optionally with the holes of that selection filled -- the module docstring has the exact rules.

    masks   as for `label`
    -> (masks, info): the cleaned masks in the input's dtype and shape (set = 1), and info = {"count": components of the input,
       "kept": components kept, "largest": area of the largest input component (0: empty mask), "area": set pixels of the output}, each
       int32 [N].  A list gives a list of masks and lists inside info.  On the device the masks are walked in chunks whose workspace
       (4 bytes per pixel per mask in flight) stays under max_workspace_bytes; nothing is read back."""
    connectivity = _check_connectivity(connectivity, "clean")
    if keep not in ("largest", "all"):
        raise RuntimeError("clean: keep must be 'largest' or 'all', got %r" % (keep,))
    if isinstance(min_area, bool) or not isinstance(min_area, (int, np.integer)) or min_area < 0:
        raise RuntimeError("clean: min_area must be an integer >= 0, got %r" % (min_area,))
    min_area = int(min(min_area, 2 ** 31 - 1))
    is_list, parts, ref = _inputs(masks, "clean")
    sizes = [0 if m is None else int(m.shape[0]) for m in parts]
    names = ("count", "kept", "largest", "area")
    if ref is None:
        return [None] * len(parts), {k: [torch.zeros(0, dtype=torch.int32) for _ in parts] for k in names}
    H, W = int(ref.shape[1]), int(ref.shape[2])
    Ntot, dev = sum(sizes), ref.device
    if not ref.is_cuda:
        m = np.concatenate([p.numpy().astype(bool) for p in parts if p is not None]) if Ntot else np.zeros((0, H, W), bool)
        if Ntot and H * W:
            o, st = _clean_np(m, connectivity, keep, min_area, bool(fill_holes))
        else:
            o, st = np.zeros((Ntot, H, W), bool), {k: np.zeros(Ntot, np.int32) for k in names}
        out = torch.from_numpy(o).to(ref.dtype)
        stats = {k: torch.from_numpy(st[k]) for k in names}
    else:
        out = _bytes_buffer(Ntot * H * W, dev).view(Ntot, H, W)
        st = torch.empty(4, Ntot, dtype=torch.int32, device=dev)
        live = [_as_bytes(p) for p in parts if p is not None and p.shape[0]]
        if Ntot and H * W:
            from ._lib import check

            def call(lib, ptrs, first, B, n, H, W, g0, ws, stream):
                s = [ctypes.c_void_p(st.data_ptr() + 4 * (k * Ntot + g0)) for k in range(4)]
                check(lib.prn_ccl_clean(_p(ptrs), _p(first), B, n, H, W, connectivity, int(keep == "all"), min_area, int(bool(fill_holes)),
                                        ctypes.c_void_p(out.data_ptr() + g0 * H * W), s[0], s[1], s[2], s[3], _p(ws), stream), "prn_ccl_clean")
            _device_run(live, "clean", max_workspace_bytes, call)
        elif Ntot:
            st.zero_()
        if ref.dtype == torch.bool:
            out = out.view(torch.bool)
        stats = {k: st[i] for i, k in enumerate(names)}
    if not is_list:
        return out, stats
    empty = torch.zeros(0, dtype=torch.int32, device=dev)
    return _split(out, sizes, parts, True), {k: [c if c is not None else empty for c in _split(v, sizes, parts, True)] for k, v in stats.items()}


@torch.no_grad()
def clean_results(results, **clean_kwargs):
    """`clean` applied to PlaneRecNet's eval-mode output (the list of per-image dicts): NEW dicts with pred_masks cleaned and pred_boxes
    recomputed from the cleaned masks (metrics.mask_boxes; an emptied mask gets that function's empty box), downloaded in one transfer
    for the batch as `inference` does -- the function's only synchronisation.  Scores, classes, depth and anything else pass through; an
    image without detections passes through; the input dicts and their tensors are not modified."""
    from .metrics import mask_boxes
    masks = [r.get("pred_masks") for r in results]
    new = [dict(r) for r in results]
    if all(m is None for m in masks):
        return new
    cleaned, _ = clean(masks, **clean_kwargs)
    live = [(b, c) for b, c in enumerate(cleaned) if c is not None and c.shape[0]]
    for b, c in enumerate(cleaned):
        if c is not None:
            new[b]["pred_masks"] = c
    if live:
        boxes = [mask_boxes(c) for _, c in live]
        host = torch.cat(boxes, 0).cpu().split([bx.shape[0] for bx in boxes])
        for (b, _), h in zip(live, host):
            new[b]["pred_boxes"] = h
    return new
