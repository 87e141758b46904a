"""Cleaning instance masks (largest connected component, holes filled): the device path (planerecnet_amd.components.clean,
csrc/prn_ccl.hip) against what a user does without it -- download the masks, then scipy.ndimage.label + bincount + binary_fill_holes per
mask (the module's own numpy path where scipy is not installed) -- alternating in one process on the same seeded inputs.

    timeout -k 10 900 python tools/components_bench.py [--reps 5] [--out profiles/components_bench.txt]

Input: 480x640 masks, one filled ellipse each with 12 specks outside it and 12 pin-holes inside it; 1 and 8 images with 10, 30 and 100 masks
each.  Prints one JSON line per measurement:
  host     download + per-mask scipy; wall clock ending in a synchronise
  device   ONE components.clean call per batch (pointer upload, workspace, ten launches per chunk); wall clock ending in a synchronise
  phases   prn_ccl_clean without the hole pass on prepared buffers, `reps x 10` back-to-back calls between two events, with the launches
           after phase k left out (include/prn.h: prn_debug_skip_launches bits 19-24); a phase's figure is the difference of two
           prefixes, so every prefix starts from the masks as a full call does.  Also the whole call with the hole pass, and prn_ccl_label.
Both paths are warmed up, measured alternately (host, device, host, device, ...) and must give equal masks.  There is no threshold: the
host figure of the same run is the yardstick."""
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

H, W = 480, 640
PHASES = ("local", "seam", "flatten", "reduce", "rank", "write")
ALL = 0x3F << 19

try:
    from scipy import ndimage
except ImportError:
    ndimage = None


def blobs(seed, n, specks=12, pinholes=12):
    """n masks: a filled ellipse each, specks outside it, pin-holes inside it (the family of tests/components_restate.py::blobs)"""
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
            m[y:y + rng.randint(1, 3), x:x + rng.randint(1, 3)] = False
        out[i] = m
    return out


def host_clean(masks):
    """what a user does today: list of device [n,H,W] bool -> list of device tensors, largest 8-connected component with its holes filled"""
    out = []
    for m in masks:
        a = m.cpu().numpy()
        if ndimage is None:
            from planerecnet_amd.components import _clean_np
            res = _clean_np(a, 8, "largest", 0, True)[0]
        else:
            res = np.zeros_like(a)
            full, cross = np.ones((3, 3), bool), ndimage.generate_binary_structure(2, 1)
            for i in range(a.shape[0]):
                lab, k = ndimage.label(a[i], structure=full)
                if k:
                    res[i] = ndimage.binary_fill_holes(lab == int(np.argmax(np.bincount(lab.ravel())[1:])) + 1, structure=cross)
        out.append(torch.from_numpy(res).to(m.device))
    return out


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


def bench(n, B, reps):
    from planerecnet_amd import components
    from planerecnet_amd._lib import check, lib
    masks = [torch.from_numpy(blobs(1000 * B + 10 * n + b, n)).cuda() for b in range(B)]

    def host():
        return host_clean(masks)

    def device():
        return components.clean(masks, 8, keep="largest", fill_holes=True, max_workspace_bytes=1 << 40)[0]

    h, d = host(), device()
    equal = all(torch.equal(a, b) for a, b in zip(h, d))
    assert equal, "host and device masks differ (n = %d, B = %d)" % (n, B)
    for _ in range(2):
        device()
    t_host, t_dev = [], []
    for _ in range(reps):                                            # alternating: both see the same machine state
        t_host.append(timed(host))
        t_dev.append(timed(device))
    host_ms, dev_ms = float(np.median(t_host)), float(np.median(t_dev))
    lines = [{"leg": "host", "n": n, "images": B, "ms": round(host_ms, 2), "min_ms": round(min(t_host), 2), "reps": reps, "scipy": ndimage is not None},
             {"leg": "device", "n": n, "images": B, "ms": round(dev_ms, 4), "min_ms": round(min(t_dev), 4), "reps": reps, "host_over_device": round(host_ms / dev_ms, 1),
              "masks_equal": equal}]
    # the launches alone, on prepared buffers
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))
    N = n * B
    m8 = [m.view(torch.uint8) for m in masks]
    ptrs = torch.tensor([m.data_ptr() for m in m8], dtype=torch.int64).cuda()
    first = torch.tensor([b * n for b in range(B + 1)], dtype=torch.int32).cuda()
    ws = torch.empty(lib.prn_ccl_ws_bytes(N, H, W) // 4 + 2, dtype=torch.int32, device="cuda")
    out = torch.empty(N * H * W // 4, dtype=torch.int32, device="cuda").view(torch.uint8).view(N, H, W)
    stats = torch.empty(4, N, dtype=torch.int32, device="cuda")
    labels = torch.empty(N, H, W, dtype=torch.int32, device="cuda")

    def clean(fill):
        check(lib.prn_ccl_clean(p(ptrs), p(first), B, N, H, W, 8, 0, 0, fill, p(out), p(stats[0]), p(stats[1]), p(stats[2]), p(stats[3]), p(ws), st), "prn_ccl_clean")

    def label():
        check(lib.prn_ccl_label(p(ptrs), p(first), B, N, H, W, 8, p(labels), p(stats[0]), p(ws), st), "prn_ccl_label")

    clean(1)
    assert torch.equal(out.view(torch.bool), torch.cat(d))
    prefix, phase_us = {}, {}
    try:
        keep, last = 0, 0.0
        for k, name in enumerate(PHASES):
            if name == "rank":
                continue                                             # (labels only)
            keep |= 1 << (19 + k)
            lib.prn_debug_skip_launches(ALL & ~keep)
            prefix[name] = events(lambda: clean(0), reps * 10)
            phase_us[name] = round(prefix[name] - last, 2)
            last = prefix[name]
    finally:
        lib.prn_debug_skip_launches(0)
    clean(1)
    assert torch.equal(out.view(torch.bool), torch.cat(d))
    lines.append({"leg": "phases", "n": n, "images": B, "us": phase_us, "clean_us": round(events(lambda: clean(0), reps * 10), 2),
                  "clean_fill_holes_us": round(events(lambda: clean(1), reps * 10), 2), "label_us": round(events(label, reps * 10), 2),
                  "mask_MB": round(N * H * W / 1e6, 2), "forest_MB": round(N * H * W * 4 / 1e6, 2)})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("components_bench.py measures on the GPU: none found")
    torch.set_num_threads(4)                                         # as eval.py
    lines = []
    for B in (1, 8):
        for n in (10, 30, 100):
            for ln in bench(n, B, a.reps):
                print(json.dumps(ln), flush=True)
                lines.append(ln)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# tools/components_bench.py --reps %d (one MI355X; %dx%d masks; host leg: %s)\n" %
                    (a.reps, H, W, "scipy.ndimage" if ndimage is not None else "the module's numpy path"))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
