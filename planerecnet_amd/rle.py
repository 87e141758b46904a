"""COCO run-length masks: the interchange format of every COCO-style tool, coded on the device (include/prn.h: prn_rle_*; DESIGN.md
section 15).

The format (pycocotools is the only other implementation and is not a dependency of this build; tests/rle_restate.py restates it loop
by loop): a mask [H,W] is walked COLUMN-major, p = x * H + y, any non-zero byte counting as set.  `counts` are the lengths of the runs of
alternating value, starting with a run of zeros (so the first count is 0 when m[0][0] is set); they sum to H * W, the odd-indexed ones to
the area.  The compressed string codes count i -- for i > 2 its difference to count i-2 -- as 5-bit groups, least significant first, one
character `chr(48 + group)` each, bit 0x20 marking that another group follows and bit 0x10 of the last group the sign.  The JSON object
is {"size": [H, W], "counts": "<string>"}; the uncompressed form carries the integer list instead.

encode() reads the masks where the model left them and downloads the strings: two blocking readbacks of per-mask size tables (run
totals, string lengths: 4 and 8 bytes per mask) and one of the packed strings, never a mask.  decode() parses on the host (vectorised
numpy) and paints on the device.  The host helpers (counts_to_string, string_to_counts, area) need no GPU.
"""
import numpy as np
import torch

from ._lib import check, lib
from ._masks import _as_bytes, _describe, _p, _stream, _upload

__all__ = ["encode", "decode", "counts_to_string", "string_to_counts", "area"]

_MAX_GROUPS = 12                                             # 5-bit groups of one value the host parser takes (60 bits; 32-bit counts need 7)


# ---------------------------------------------------------------------------------------------------------------- host helpers
def counts_to_string(counts):
    """run lengths (a sequence of non-negative ints) -> the compressed string.  Vectorised over the counts: one numpy pass per 5-bit
    group position, none per count or per character."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if c.size == 0:
        return ""
    if (c < 0).any():
        raise ValueError("counts must not be negative")
    x = c.copy()
    x[3:] -= c[1:-2]
    chars = np.zeros((c.size, 13), np.uint8)                 # (13 groups: any int64 difference)
    alive = np.ones(c.size, bool)
    keep = np.zeros((c.size, 13), bool)
    for k in range(13):
        g = x & 0x1f
        x = x >> 5                                           # arithmetic
        more = np.where(g & 0x10, x != -1, x != 0)
        keep[:, k] = alive
        chars[:, k] = (g | np.where(more, 0x20, 0)) + 48
        alive = alive & more
        if not alive.any():
            break
    return chars[keep].tobytes().decode("ascii")


def string_to_counts(s):
    """the compressed string (str or bytes) -> run lengths, int64 array.  Vectorised: the groups of one value are summed with one
    `np.add.reduceat`, the recurrence over count i-2 is two strided cumulative sums.  ValueError: a character outside the 64 the format
    uses, a string whose last character announces another group (truncated), a value of more than 60 bits."""
    b = s.encode("ascii") if isinstance(s, str) else bytes(s)
    a = np.frombuffer(b, dtype=np.uint8).astype(np.int64) - 48
    if a.size == 0:
        return np.zeros(0, np.int64)
    if ((a < 0) | (a > 63)).any():
        raise ValueError("not a COCO run-length string: character outside chr(48) .. chr(111)")
    more = (a & 0x20) != 0
    if more[-1]:
        raise ValueError("truncated run-length string: the last character announces another group")
    start = np.flatnonzero(np.concatenate(([True], ~more[:-1])))          # first character of every value
    length = np.diff(np.concatenate((start, [a.size])))
    k = np.arange(a.size) - np.repeat(start, length)                      # group position inside its value
    if (length > _MAX_GROUPS).any():
        raise ValueError("not a COCO run-length string: a value of more than %d bits" % (5 * _MAX_GROUPS))
    x = np.add.reduceat((a & 0x1f) << (5 * k), start)
    last = a[start + length - 1]
    x = np.where(last & 0x10, x - (np.int64(1) << (5 * length)), x)       # sign extension from the last group
    c = x.copy()
    c[1::2] = np.cumsum(x[1::2])                                          # counts 1, 3, 5, ...: each adds to the one two before it
    c[2::2] = np.cumsum(x[2::2])                                          # counts 2, 4, 6, ... likewise; count 0 stands alone
    return c


def _counts_of(rle):
    c = rle["counts"]
    if isinstance(c, (str, bytes, bytearray)):
        return string_to_counts(c)
    c = np.asarray(c)
    if c.size and c.dtype.kind not in "iu":
        raise ValueError("uncompressed counts must be integers, got %s" % c.dtype)
    return c.astype(np.int64).reshape(-1)


def area(rle):
    """set pixels of one RLE dict: the sum of its odd-indexed counts"""
    return int(_counts_of(rle)[1::2].sum())


# ---------------------------------------------------------------------------------------------------------------- encode
def _mask_list(masks):
    """-> (per image: a contiguous uint8 [N_b,H,W] device tensor, or None where the image has no instances; the first of those tensors)"""
    out, ref, hw = [], None, None
    for b, m in enumerate(masks):
        if m is None:
            out.append(None)
            continue
        if not (torch.is_tensor(m) and m.dtype in (torch.bool, torch.uint8) and m.dim() == 3):
            raise RuntimeError("masks[%d] must be a bool / uint8 [N,H,W] tensor, got %s" % (b, _describe(m)))
        if hw is None:
            hw = tuple(m.shape[1:])
        elif tuple(m.shape[1:]) != hw:
            raise RuntimeError("masks[%d] is %s: every image must have the same H and W %s" % (b, tuple(m.shape), hw))
        if int(m.shape[0]) == 0:
            out.append(None)
            continue
        if not m.is_cuda or (ref is not None and m.device != ref.device):
            raise RuntimeError("masks[%d] must be a device tensor%s (the codec has no host path), got %s" %
                               (b, "" if ref is None else " on %s" % ref.device, _describe(m)))
        m = _as_bytes(m)
        ref = m if ref is None else ref
        out.append(m)
    return out, ref


@torch.no_grad()
def encode(masks):
    """Instance masks -> COCO RLE dicts {"size": [H, W], "counts": str}, coded on the device.

    masks  a [N,H,W] bool / uint8 device tensor (non-zero = set) -> a list of N dicts;
           or a list of B such tensors of one H, W (None or N = 0: an image without instances) -> a list of B such lists.
    Non-contiguous inputs are made contiguous.  Host traffic: the per-mask run totals (blocking), the per-mask string lengths (blocking),
    the packed strings; never the masks.  No instances at all: nothing is launched.  Deterministic (no atomics)."""
    single = torch.is_tensor(masks)
    ms, ref = _mask_list([masks] if single else list(masks))
    sizes = [0 if m is None else int(m.shape[0]) for m in ms]
    ntot = sum(sizes)
    if ntot == 0:
        return [] if single else [[] for _ in ms]
    H, W = int(ref.shape[1]), int(ref.shape[2])
    if H <= 0 or W <= 0 or H * W >= 1 << 31:
        raise RuntimeError("masks must have 0 < H * W < 2^31, got H=%d W=%d" % (H, W))
    dev = ref.device
    B = len(ms)
    first = [0]
    for n in sizes:
        first.append(first[-1] + n)
    with torch.cuda.device(dev):
        st = _stream(dev)
        ptrs = _upload([0 if m is None else m.data_ptr() for m in ms], torch.int64, dev)
        first_dev = _upload(first, torch.int32, dev)
        ws = torch.empty(lib.prn_rle_ws_bytes(ntot, H, W) // 4, dtype=torch.int32, device=dev)
        totals = torch.empty(ntot, dtype=torch.int32, device=dev)
        check(lib.prn_rle_count(_p(ptrs), _p(first_dev), B, ntot, H, W, _p(ws), _p(totals), st), "prn_rle_count")
        pos_first = np.concatenate(([0], np.cumsum(totals.cpu().numpy().astype(np.int64))))            # readback 1: boundaries per mask
        pos_first_dev = _upload(pos_first.tolist(), torch.int64, dev)
        pos = torch.empty(max(int(pos_first[-1]), 1), dtype=torch.int32, device=dev)
        check(lib.prn_rle_fill(_p(ptrs), _p(first_dev), B, ntot, H, W, _p(ws), _p(pos_first_dev), _p(pos), st), "prn_rle_fill")
        str_len = torch.empty(ntot, dtype=torch.int64, device=dev)
        check(lib.prn_rle_string_lengths(_p(pos), _p(pos_first_dev), ntot, H, W, _p(str_len), st), "prn_rle_string_lengths")
        str_first = np.concatenate(([0], np.cumsum(str_len.cpu().numpy())))                             # readback 2: characters per mask
        str_first_dev = _upload(str_first.tolist(), torch.int64, dev)
        packed = torch.empty(int(str_first[-1]), dtype=torch.uint8, device=dev)
        check(lib.prn_rle_strings(_p(pos), _p(pos_first_dev), _p(str_first_dev), ntot, H, W, _p(packed), st), "prn_rle_strings")
        text = packed.cpu().numpy().tobytes().decode("ascii")                                           # the one download of the answer
    rles = [{"size": [H, W], "counts": text[int(str_first[n]):int(str_first[n + 1])]} for n in range(ntot)]
    if single:
        return rles
    return [rles[first[b]:first[b + 1]] for b in range(B)]


# ---------------------------------------------------------------------------------------------------------------- decode
def _parse(rles):
    """validated host tables of a list of RLE dicts: (H, W, ends uint32 [sum of runs], end_first int64 [N+1]); ValueError on a bad input"""
    H = W = None
    ends, end_first = [], [0]
    for i, r in enumerate(rles):
        size = r["size"]
        if len(size) != 2 or int(size[0]) <= 0 or int(size[1]) <= 0:
            raise ValueError("rles[%d]: size must be two positive ints, got %r" % (i, size))
        h, w = int(size[0]), int(size[1])
        if H is None:
            H, W = h, w
        elif (h, w) != (H, W):
            raise ValueError("rles[%d] has size %r, the others [%d, %d]: all sizes must agree" % (i, size, H, W))
        if H * W >= 1 << 31:
            raise ValueError("rles[%d]: H * W = %d does not index in 31 bits" % (i, H * W))
        c = _counts_of(r)
        if (c < 0).any():
            raise ValueError("rles[%d]: negative count" % i)
        total = int(np.minimum(c, H * W + 1).sum())                           # (clipped: no count of a valid list exceeds H * W, and the sum cannot wrap)
        if total != H * W:
            raise ValueError("rles[%d]: the counts sum to %s, not to H * W = %d" % (i, total if total <= H * W else "more than %d" % (H * W), H * W))
        ends.append(np.cumsum(c).astype(np.uint32))
        end_first.append(end_first[-1] + c.size)
    return H, W, ends, end_first


@torch.no_grad()
def decode(rles, device):
    """A list of N RLE dicts ({"size": [H, W], "counts": str | bytes | list of ints}, all of one size) -> uint8 [N,H,W] tensor on `device`
    (1 = set).  Strings are parsed on the host; ValueError BEFORE any launch for a negative count, counts that do not sum to H * W, a
    truncated string (continuation bit on its last character), characters outside the format, or differing sizes.  N = 0: RuntimeError,
    there is no size to give the result."""
    rles = list(rles)
    if not rles:
        raise RuntimeError("decode needs at least one RLE (an empty list has no size)")
    H, W, ends, end_first = _parse(rles)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("decode paints on the device (the codec has no host path), got device %s" % (dev,))
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        e_dev = torch.from_numpy(np.concatenate(ends).view(np.int32)).pin_memory().to(dev, non_blocking=True)
        f_dev = _upload(end_first, torch.int64, dev)
        out = torch.empty(len(rles), H, W, dtype=torch.uint8, device=dev)
        check(lib.prn_rle_paint(_p(e_dev), _p(f_dev), len(rles), H, W, _p(out), _stream(dev)), "prn_rle_paint")
    return out
