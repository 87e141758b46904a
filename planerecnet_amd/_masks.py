"""What the Python wrappers of the mask operators share (csrc/prn_masks.h is the device side): argument plumbing for the C calls, the checks
of a ragged batch of [N,H,W] masks, and the walk of such a batch in chunks a workspace limit admits.  Private: no public API."""
import ctypes

import torch

MAX_MASKS = 65535        # masks per library call (the grid's y)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _upload(values, dtype, device):
    """host values -> device tensor through page-locked memory (an asynchronous copy: no host synchronisation)"""
    return torch.tensor(values, dtype=dtype).pin_memory().to(device, non_blocking=True)


def _stream(device):
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(device.index))


def _describe(t):
    return "%s %s %s" % (t.device, t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__


def _bytes_buffer(n, device):
    """n bytes as a view of an int32 allocation (4-byte allocations are what the suite's guard mode brackets)"""
    return torch.empty((n + 3) // 4, dtype=torch.int32, device=device).view(torch.uint8)[:n]


def _as_bytes(m):
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _inputs(masks, what):
    """-> (is_list, parts, ref): parts[b] = None or a [N_b,H,W] bool / uint8 tensor; one device, one dtype, one H x W; ref = the first tensor"""
    is_list = isinstance(masks, (list, tuple))
    parts = list(masks) if is_list else [masks]
    ref = None
    for b, m in enumerate(parts):
        if m is None and is_list:
            continue
        if not (torch.is_tensor(m) and m.dim() == 3 and m.dtype in (torch.bool, torch.uint8)):
            raise RuntimeError("%s: masks%s must be a bool / uint8 [N,H,W] tensor, got %s" % (what, "[%d]" % b if is_list else "", _describe(m)))
        if ref is None:
            ref = m
        elif m.device != ref.device or m.dtype != ref.dtype or m.shape[1:] != ref.shape[1:]:
            raise RuntimeError("%s: masks[%d] is %s, masks before it %s (one device, dtype and H x W per call)" % (what, b, _describe(m), _describe(ref)))
    return is_list, parts, ref


def _split(t, sizes, parts, is_list):
    """a per-mask tensor over the non-empty images -> per-image outputs in input order (None stays None, N_b = 0 gives an empty tensor)"""
    if not is_list:
        return t
    out, o = [], 0
    for m, n in zip(parts, sizes):
        if m is None:
            out.append(None)
        else:
            out.append(t[o:o + n])
            o += n
    return out


def ragged_chunks(parts, per_mask_bytes, max_workspace_bytes):
    """parts: contiguous uint8 [N_b,H,W] device tensors with N_b > 0.  Their masks as chunks whose workspace (per_mask_bytes each) stays under
    the limit: yields (g0, g1, ptrs, first) -- the global mask range, device tables of the byte address of each contributing image's first
    mask in the range and of their running counts (prn_mask_src).  A chunk may span images and an image several chunks; sizes are host
    knowledge, so nothing is read back."""
    dev = parts[0].device
    HW = int(parts[0].shape[1]) * int(parts[0].shape[2])
    cap = int(max(1, min(MAX_MASKS, int(max_workspace_bytes) // per_mask_bytes)))
    first = [0]
    for m in parts:
        first.append(first[-1] + int(m.shape[0]))
    for g0 in range(0, first[-1], cap):
        g1 = min(first[-1], g0 + cap)
        ptrs, cnt = [], [0]
        for b, m in enumerate(parts):
            lo, hi = max(g0, first[b]), min(g1, first[b + 1])
            if lo < hi:
                ptrs.append(m.data_ptr() + (lo - first[b]) * HW)
                cnt.append(cnt[-1] + hi - lo)
        yield g0, g1, _upload(ptrs, torch.int64, dev), _upload(cnt, torch.int32, dev)
