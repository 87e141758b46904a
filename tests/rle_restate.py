"""The COCO run-length mask format, restated loop by loop from its definition (planerecnet_amd/rle.py: module docstring).  Deliberately
slow and plain -- one Python step per pixel, per count and per character -- and independent of rle.py's vectorised host code and of the
device kernels: it is what both are tested against, together with the hand-derived vectors of tests/golden/coco_rle_vectors.json."""
import json
import os

import numpy as np


def mask_to_counts(mask):
    """mask [H][W] (anything indexable, non-zero = set) -> run lengths of alternating value in column-major order, starting with zeros"""
    m = np.asarray(mask)
    H, W = m.shape
    m = m.tolist()                                           # (plain lists: the loop below indexes every pixel)
    counts = []
    value, run = 0, 0
    for x in range(W):
        for y in range(H):                                   # p = x * H + y
            v = 1 if m[y][x] != 0 else 0
            if v != value:
                counts.append(run)
                value, run = v, 0
            run += 1
    counts.append(run)
    return counts


def counts_to_mask(counts, H, W):
    """run lengths -> uint8 mask [H][W]"""
    m = np.zeros((H, W), np.uint8)
    p, value = 0, 0
    for c in counts:
        for _ in range(int(c)):
            m[p % H][p // H] = value
            p += 1
        value = 1 - value
    assert p == H * W, (p, H, W)
    return m


def counts_to_string(counts):
    out = []
    for i in range(len(counts)):
        x = int(counts[i])
        if i > 2:
            x -= int(counts[i - 2])
        while True:
            c = x & 0x1f
            x >>= 5                                          # (Python's >> on a negative int is arithmetic)
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
            if not more:
                break
    return "".join(out)


def string_to_counts(s):
    if isinstance(s, bytes):
        s = s.decode("ascii")
    counts = []
    p = 0
    while p < len(s):
        x, k = 0, 0
        while True:
            if p >= len(s):
                raise ValueError("truncated")
            c = ord(s[p]) - 48
            p += 1
            x |= (c & 0x1f) << (5 * k)
            k += 1
            if not (c & 0x20):
                if c & 0x10:
                    x |= -1 << (5 * k)
                break
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def area(counts):
    total = 0
    for i in range(1, len(counts), 2):
        total += int(counts[i])
    return total


# ---- the fixture file: tests/golden/coco_rle_vectors.json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_vectors():
    with open(os.path.join(ROOT, "tests", "golden", "coco_rle_vectors.json")) as f:
        return json.load(f)


def build_mask(size, spec):
    """the mask a fixture entry describes (entries without "mask" are given by their counts alone)"""
    H, W = size
    m = np.zeros((H, W), np.uint8)
    kind = spec["kind"]
    if kind == "ones":
        m[:] = 1
    elif kind == "points":
        for y, x in spec["points"]:
            m[y][x] = 1
    elif kind == "rect":
        m[spec["rows"][0]:spec["rows"][1] + 1, spec["cols"][0]:spec["cols"][1] + 1] = 1
    elif kind == "checker":
        yy, xx = np.mgrid[:H, :W]
        m = ((xx + yy) & 1).astype(np.uint8)
    else:
        assert kind == "zeros", kind
    return m
