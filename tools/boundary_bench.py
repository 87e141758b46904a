"""Boundary IoU of a frame's detections against its ground truth: the device path (planerecnet_amd.metrics.boundary_iou,
planerecnet_amd.morphology.boundary; csrc/prn_morph.hip) against what a user does without it -- download both mask sets,
scipy.ndimage.binary_erosion per mask, IoU matrices in numpy -- alternating in one process on the same seeded inputs, and against
metrics.pairwise_iou alone (the difference is what `eval.py --boundary_ap` adds per frame).

    timeout -k 10 900 python tools/boundary_bench.py [--reps 5] [--out profiles/boundary_bench.txt]

Input: one filled ellipse per mask with specks and pin-holes, at 480 x 640 (radius 16) and 736 x 960 (radius 24), (A, B) = (10, 10), (20, 15),
(100, 30).  Prints one JSON line per measurement:
  host      download + per-mask scipy erosion + numpy IoU (mask and boundary); wall clock ending in a synchronise
  device    ONE metrics.boundary_iou call (workspace, seven launches); wall clock ending in a synchronise; `pairwise_ms` is metrics.pairwise_iou
            of the masks alone, measured in the same alternation
  band      ONE morphology.boundary call on the A + B masks (pointer upload, workspace, three launches, bytes written)
  phases    prn_boundary_iou on prepared buffers, `reps x 10` back-to-back calls between two events, with the launches after phase k left
            out (include/prn.h: prn_debug_skip_launches bits 25-28); a phase's figure is the difference of two prefixes
All legs are warmed up and measured alternately; host and device matrices must be equal bit for bit.  There is no threshold: the host
figure of the same run is the yardstick."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("pack", "row", "column", "pairs")
ALL = 0xF << 25

try:
    from scipy import ndimage
except ImportError:
    ndimage = None


def blobs(seed, n, H, W, specks=12, pinholes=12):
    """n masks: a filled ellipse each, specks outside it, pin-holes inside it"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((n, H, W), bool)
    for i in range(n):
        cy, cx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W
        ry, rx = rng.uniform(0.08, 0.3) * H + 1, rng.uniform(0.08, 0.3) * W + 1
        m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        inside = np.flatnonzero(m)
        for _ in range(specks):
            y, x = rng.randint(H), rng.randint(W)
            m[y:y + rng.randint(1, 4), x:x + rng.randint(1, 4)] = True
        for p in rng.choice(inside, min(pinholes, inside.size), replace=False):
            y, x = divmod(int(p), W)
            m[y, x] = False
        out[i] = m
    return out


def iou_f32(a, b):
    fa, fb = a.reshape(len(a), -1).astype(np.float32), b.reshape(len(b), -1).astype(np.float32)
    inter = fa @ fb.T                                                 # (0/1 products, sums below 2^24: exact)
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / ((fa.sum(1)[:, None] + fb.sum(1)[None, :]) - inter)


def host_boundary_iou(a, b, r):
    """what a user does today: device [A,H,W], [B,H,W] bool -> (mask IoU, boundary IoU) as numpy fp32"""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    if ndimage is None:
        from planerecnet_amd.morphology import _morph_np
        ba, bb = _morph_np(a, 2, r, 0), _morph_np(b, 2, r, 0)
    else:
        full = np.ones((3, 3), bool)
        ba = np.stack([m & ~ndimage.binary_erosion(m, full, iterations=r, border_value=0) for m in a])
        bb = np.stack([m & ~ndimage.binary_erosion(m, full, iterations=r, border_value=0) for m in b])
    return iou_f32(a, b), iou_f32(ba, bb)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3                          # microseconds per call


def bench(H, W, A, B, reps):
    from planerecnet_amd import metrics, morphology
    from planerecnet_amd._lib import check, lib
    r = morphology.boundary_radius(H, W)
    a = torch.from_numpy(blobs(H + 10 * A, A, H, W)).cuda()
    b = torch.from_numpy(blobs(W + 10 * B, B, H, W)).cuda()

    def host():
        return host_boundary_iou(a, b, r)

    def device():
        return metrics.boundary_iou(a, b, radius=r)

    def pairwise():
        return metrics.pairwise_iou(a, b)[0]

    def band():
        return morphology.boundary([a, b], r)

    (hm, hb), (dm, db) = host(), device()
    equal = np.array_equal(hm, dm.cpu().numpy(), equal_nan=True) and np.array_equal(hb, db.cpu().numpy(), equal_nan=True)
    assert equal, "host and device matrices differ (%d x %d, A = %d, B = %d)" % (H, W, A, B)
    for _ in range(2):
        device(), pairwise(), band()
    t = {"host": [], "device": [], "pairwise": [], "band": []}
    for _ in range(reps):                                            # alternating: all see the same machine state
        for name, fn in (("host", host), ("device", device), ("pairwise", pairwise), ("band", band)):
            t[name].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in t.items()}
    tag = {"size": "%dx%d" % (H, W), "radius": r, "A": A, "B": B, "reps": reps}
    lines = [dict(tag, leg="host", ms=round(med["host"], 2), min_ms=round(min(t["host"]), 2), scipy=ndimage is not None),
             dict(tag, leg="device", ms=round(med["device"], 4), min_ms=round(min(t["device"]), 4), pairwise_ms=round(med["pairwise"], 4),
                  added_ms=round(med["device"] - med["pairwise"], 4), host_over_device=round(med["host"] / med["device"], 1), matrices_equal=equal),
             dict(tag, leg="band", ms=round(med["band"], 4), min_ms=round(min(t["band"]), 4))]
    # the launches alone, on prepared buffers
    p = lambda x: ctypes.c_void_p(x.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))
    a8, b8 = a.view(torch.uint8), b.view(torch.uint8)
    out = torch.empty(2, A, B, device="cuda")
    ws = torch.empty(lib.prn_boundary_iou_ws_bytes(A, B, H, W) // 4 + 2, dtype=torch.int32, device="cuda")

    def call():
        check(lib.prn_boundary_iou(p(a8), p(b8), A, B, H, W, r, p(out[0]), p(out[1]), p(ws), st), "prn_boundary_iou")

    call()
    assert torch.equal(out[1].view(torch.int32), db.view(torch.int32))
    prefix, phase_us, keep, last = {}, {}, 0, 0.0
    try:
        for k, name in enumerate(PHASES):
            keep |= 1 << (25 + k)
            lib.prn_debug_skip_launches(ALL & ~keep)
            prefix[name] = events(call, reps * 10)
            phase_us[name] = round(prefix[name] - last, 2)
            last = prefix[name]
    finally:
        lib.prn_debug_skip_launches(0)
    call()
    assert torch.equal(out[1].view(torch.int32), db.view(torch.int32))
    lines.append(dict(tag, leg="phases", us=phase_us, call_us=round(events(call, reps * 10), 2), mask_MB=round((A + B) * H * W / 1e6, 2),
                      packed_MB=round((A + B) * H * ((W + 63) // 64) * 8 / 1e6, 3)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boundary_bench.py measures on the GPU: none found")
    torch.set_num_threads(4)                                         # as eval.py
    lines = []
    for H, W in ((480, 640), (736, 960)):
        for A, B in ((10, 10), (20, 15), (100, 30)):
            for ln in bench(H, W, A, B, a.reps):
                print(json.dumps(ln), flush=True)
                lines.append(ln)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# tools/boundary_bench.py --reps %d (one MI355X; host leg: %s)\n" % (a.reps, "scipy.ndimage" if ndimage is not None else "the module's numpy path"))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
