"""Greedy mask NMS (`--nms_mode mask`) of one post-process: the device path (planerecnet_amd.nms.mask_nms_batched, csrc/prn_mask_nms.hip)
against the host path it replaced (copied below as it stood: an fp32 copy of the masks times its transpose through ATen, the [n, n] suppression
matrix downloaded, a Python double loop), alternating in one process on the same seeded inputs.

    timeout -k 10 900 python tools/mask_nms_bench.py [--reps 5] [--out profiles/mask_nms_bench.txt]

Input: 120x160 masks (the mask head's size at 480x640), rectangles clustered round n/4 centres with 5 % of their pixels knocked out, two labels,
n = 100, 300 and 500 (nms_pre) candidates per image; one image and a batch of 8 (the host path has no batched form: it runs per image).
Prints one JSON line per measurement:
  host     the former mask_nms per image; wall clock ending in a synchronise
  device   ONE mask_nms_batched call (offset upload, workspace, three launches, the cast of `keep`); wall clock ending in a synchronise
  stages   each of the three launches alone, `reps x 10` back-to-back launches between two events, on the buffers a full call left
           (include/prn.h: prn_debug_skip_launches bits 16-18)
Both paths are warmed up, measured alternately (host, device, host, device, ...) and must give equal `keep` vectors.  There is no
threshold: the host figure of the same run is the yardstick."""
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

H, W = 120, 160


def host_mask_nms(cate_labels, seg_masks, sum_masks, cate_scores, nms_thr=0.5):
    """planerecnet_amd/nms.py::mask_nms before the device path, verbatim"""
    n = len(cate_scores)
    if n == 0:
        return []
    flat = seg_masks.reshape(n, -1).float()
    inter = flat @ flat.t()
    union = sum_masks[:, None] + sum_masks[None, :] - inter
    same = cate_labels[:, None] == cate_labels[None, :]
    suppress = (same & ((union <= 0) | (inter / union.clamp(min=1e-12) > nms_thr))).cpu()
    keep = [True] * n
    for i in range(n - 1):
        if keep[i]:
            for j in range(i + 1, n):
                if keep[j] and suppress[i, j]:
                    keep[j] = False
    return torch.tensor(keep, device=seg_masks.device).to(seg_masks.dtype)


def clustered(seed, n):
    """-> (labels int64 [n], masks bool [n,H,W], sums fp32 [n]) in descending score order (the family of tests/mask_nms_restate.py)"""
    rng = np.random.RandomState(seed)
    nc = max(1, n // 4)
    cy, cx = rng.randint(0, H, nc), rng.randint(0, W, nc)
    bh, bw = rng.randint(H // 8, H // 3 + 1, nc), rng.randint(W // 8, W // 3 + 1, nc)
    masks = np.zeros((n, H, W), bool)
    which = rng.randint(0, nc, n)
    for m in range(n):
        c = which[m]
        y0, x0 = cy[c] - bh[c] // 2 + rng.randint(-7, 8), cx[c] - bw[c] // 2 + rng.randint(-10, 11)
        y1, x1 = y0 + max(1, bh[c] + rng.randint(-7, 8)), x0 + max(1, bw[c] + rng.randint(-10, 11))
        masks[m, max(0, y0):max(0, y1), max(0, x0):max(0, x1)] = True
        masks[m] &= rng.rand(H, W) >= 0.05
    return rng.randint(0, 2, n).astype(np.int64), masks, masks.reshape(n, H * W).sum(1).astype(np.float32)


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


def bench(n, B, reps, thr=0.5):
    from planerecnet_amd import nms
    from planerecnet_amd._lib import check, lib
    parts = [clustered(1000 * B + 10 * n + b, n) for b in range(B)]
    labels, masks, sums = (torch.from_numpy(np.concatenate([p[k] for p in parts])).cuda() for k in range(3))
    counts = [n] * B
    scores = torch.zeros(n, device="cuda")

    def host():
        return torch.cat([host_mask_nms(labels[b * n:(b + 1) * n], masks[b * n:(b + 1) * n], sums[b * n:(b + 1) * n], scores, thr) for b in range(B)])

    def device():
        return nms.mask_nms_batched(labels, masks, sums, counts, nms_thr=thr)

    h, d = host(), device()
    equal = bool(torch.equal(h, d))
    assert equal, "host and device keep vectors differ (n = %d, B = %d)" % (n, B)
    for _ in range(2):
        device()
    t_host, t_dev = [], []
    for _ in range(reps):                                            # alternating: both see the same machine state
        t_host.append(timed(host))
        t_dev.append(timed(device))
    host_ms, dev_ms = float(np.median(t_host)), float(np.median(t_dev))
    lines = [{"leg": "host", "n": n, "images": B, "ms": round(host_ms, 3), "min_ms": round(min(t_host), 3), "reps": reps},
             {"leg": "device", "n": n, "images": B, "ms": round(dev_ms, 4), "min_ms": round(min(t_dev), 4), "reps": reps, "host_over_device": round(host_ms / dev_ms, 1),
              "keep_equal": equal, "kept": int(d.sum()), "of": n * B}]
    # the launches alone, on prepared buffers
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))
    m8 = masks.contiguous().view(torch.uint8)
    seg = torch.tensor([b * n for b in range(B + 1)], dtype=torch.int32).cuda()
    ws = torch.empty(lib.prn_mask_nms_ws_bytes(n * B, n, H * W) // 4 + 2, dtype=torch.float32, device="cuda")
    keep = torch.empty(n * B, dtype=torch.uint8, device="cuda")
    run = lambda: check(lib.prn_mask_nms(p(m8), p(labels), p(sums), p(seg), B, n, H * W, thr, p(keep), p(ws), st), "prn_mask_nms")      # noqa: E731
    run()
    assert torch.equal(keep.bool(), d)
    stage_us = {}
    try:
        for name, others in (("pack", 6), ("pairs", 5), ("sweep", 3)):
            lib.prn_debug_skip_launches(others << 16)
            stage_us[name] = round(events(run, reps * 10), 2)
    finally:
        lib.prn_debug_skip_launches(0)
    run()
    assert torch.equal(keep.bool(), d)
    lines.append({"leg": "stages", "n": n, "images": B, "us": stage_us, "all_three_us": round(events(run, reps * 10), 2),
                  "mask_MB": round(n * B * H * W / 1e6, 2), "packed_MB": round(n * B * H * W / 8e6, 3)})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_nms_bench.py measures on the GPU: none found")
    torch.set_num_threads(4)                                         # as eval.py
    lines = []
    for B in (1, 8):
        for n in (100, 300, 500):
            for ln in bench(n, B, a.reps):
                print(json.dumps(ln), flush=True)
                lines.append(ln)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# tools/mask_nms_bench.py --reps %d (one MI355X; %dx%d masks)\n" % (a.reps, H, W))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
