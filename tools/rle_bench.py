"""COCO run-length encoding of one frame's instance masks: the device path (planerecnet_amd.rle.encode, csrc/prn_rle.hip; what comes
back to the host are the strings) against the honest host path (download of the masks, a VECTORISED numpy encoder, the module's own
counts_to_string), in one process on one seeded synthetic result.

    timeout -k 10 600 python tools/rle_bench.py [--reps 10] [--out profiles/rle_bench.txt]

Input: 480x640, N = 100 and N = 20 instance masks (rectangles and ellipses of 1-12 % of the frame, 5 % holes: tools/render_bench.py's).
Prints one JSON line per measurement:
  host     masks.cpu() + per mask np.flatnonzero of the column-major difference, np.diff, rle.counts_to_string; wall clock per frame
           (its parts too: the download alone, the run extraction alone, the strings alone)
  device   rle.encode(masks) including its two size readbacks and the download of the strings; wall clock per frame
  kernels  each launch alone on prepared buffers, `reps x 10` back-to-back launches between two events; the bytes the launch has to move
           over that time against the 6.3 TB/s copy rate of the MI355X
There is no threshold: the host figure of the same run is the yardstick."""
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
from tools.render_bench import COPY_TBPS, H, W, events, make_result, rate, wall  # noqa: E402


def host_counts(mask):
    """one [H,W] bool mask -> run lengths, vectorised: the positions where the column-major sequence changes, differenced"""
    flat = np.asfortranarray(mask).reshape(-1, order="F").view(np.uint8)
    edge = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    ends = np.concatenate(([0] if flat[0] == 0 else [0, 0], edge, [flat.size]))
    return np.diff(ends)


def bench(N, reps):
    from planerecnet_amd import rle
    from planerecnet_amd._lib import check, lib
    result, _ = make_result(N)
    masks = result["pred_masks"]
    lines = []

    def host():
        m = masks.cpu().numpy()
        return [{"size": [H, W], "counts": rle.counts_to_string(host_counts(m[i]))} for i in range(N)]

    def device():
        return rle.encode(masks)

    h, d = host(), device()
    same = h == d
    m_host = masks.cpu().numpy()
    counts = [host_counts(m_host[i]) for i in range(N)]
    host_ms, dev_ms = wall(host, max(3, reps), 1), wall(device, reps * 3, 3)
    parts = {"download_ms": wall(lambda: masks.cpu(), max(3, reps), 1), "runs_ms": wall(lambda: [host_counts(m_host[i]) for i in range(N)], max(3, reps), 1),
             "strings_ms": wall(lambda: [rle.counts_to_string(c) for c in counts], max(3, reps), 1)}
    nruns = sum(len(c) for c in counts)
    nchars = sum(len(r["counts"]) for r in d)
    lines.append(dict({"leg": "host", "N": N, "H": H, "W": W, "ms_per_frame": round(host_ms, 3)}, **{k: round(v, 3) for k, v in parts.items()}))
    lines.append({"leg": "device", "N": N, "H": H, "W": W, "ms_per_frame": round(dev_ms, 3), "host_over_device": round(host_ms / dev_ms, 2),
                  "strings_equal_host": same, "counts": nruns, "characters": nchars, "mask_MB": round(N * H * W / 1e6, 2),
                  "note": "includes the pointer-table uploads, the allocations, two blocking size readbacks and the download of the strings"})
    # the launches alone, on prepared buffers
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))
    m = masks.contiguous().view(torch.uint8)
    ptrs = torch.tensor([m.data_ptr()], dtype=torch.int64).cuda()
    first = torch.tensor([0, N], dtype=torch.int32).cuda()
    ws = torch.empty(lib.prn_rle_ws_bytes(N, H, W) // 4, dtype=torch.int32, device="cuda")
    totals = torch.empty(N, dtype=torch.int32, device="cuda")
    run = lambda: check(lib.prn_rle_count(p(ptrs), p(first), 1, N, H, W, p(ws), p(totals), st), "count")      # noqa: E731
    run()
    pos_first = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), totals.long().cumsum(0)])
    K = int(pos_first[-1])
    pos = torch.empty(max(K, 1), dtype=torch.int32, device="cuda")
    cells = ws.numel() * 4
    us = events(run, reps * 10)
    lines.append(dict({"leg": "count + scan", "N": N, "launches": 2, "bytes": "N H W mask bytes + the cell table written, read and rewritten"},
                      **rate(N * H * W + 3 * cells, us)))
    fill = lambda: check(lib.prn_rle_fill(p(ptrs), p(first), 1, N, H, W, p(ws), p(pos_first), p(pos), st), "fill")      # noqa: E731
    run()                                                             # (prn_rle_fill reads the ranks the count step left)
    us = events(fill, reps * 10)
    lines.append(dict({"leg": "fill", "N": N, "launches": 1, "bytes": "N H W mask bytes + the cell table + 4 bytes per boundary"}, **rate(N * H * W + cells + 4 * K, us)))
    str_len = torch.empty(N, dtype=torch.int64, device="cuda")
    lens = lambda: check(lib.prn_rle_string_lengths(p(pos), p(pos_first), N, H, W, p(str_len), st), "lengths")      # noqa: E731
    lens()
    us = events(lens, reps * 10)
    lines.append(dict({"leg": "string lengths", "N": N, "launches": 1, "bytes": "4 bytes per boundary"}, **rate(4 * K, us)))
    str_first = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), str_len.cumsum(0)])
    packed = torch.empty(int(str_first[-1]), dtype=torch.uint8, device="cuda")
    strs = lambda: check(lib.prn_rle_strings(p(pos), p(pos_first), p(str_first), N, H, W, p(packed), st), "strings")      # noqa: E731
    us = events(strs, reps * 10)
    lines.append(dict({"leg": "strings", "N": N, "launches": 1, "bytes": "4 bytes per boundary + the characters"}, **rate(4 * K + packed.numel(), us)))
    # decoding: the painter on the same masks' run ends
    ends = [np.cumsum(c).astype(np.uint32) for c in counts]
    e_dev = torch.from_numpy(np.concatenate(ends).view(np.int32)).cuda()
    f_dev = torch.tensor(np.concatenate(([0], np.cumsum([len(e) for e in ends]))).tolist(), dtype=torch.int64).cuda()
    out = torch.empty(N, H, W, dtype=torch.uint8, device="cuda")
    paint = lambda: check(lib.prn_rle_paint(p(e_dev), p(f_dev), N, H, W, p(out), st), "paint")      # noqa: E731
    paint()
    painted_equal = bool(torch.equal(out, m))
    us = events(paint, reps * 10)
    lines.append(dict({"leg": "paint", "N": N, "launches": 1, "equals_masks": painted_equal, "bytes": "N H W bytes written + 4 bytes per run end"},
                      **rate(N * H * W + 4 * e_dev.numel(), us)))
    lines.append({"leg": "decode", "N": N, "ms_per_frame": round(wall(lambda: rle.decode(d, "cuda:0"), reps * 3, 3), 3),
                  "note": "rle.decode of the strings: host parsing, upload of the run ends, the painter (no download)"})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rle_bench.py measures on the GPU: none found")
    torch.set_num_threads(4)                                         # as eval.py
    lines = []
    for N in (100, 20):
        for ln in bench(N, a.reps):
            print(json.dumps(ln), flush=True)
            lines.append(ln)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# tools/rle_bench.py --reps %d (one MI355X; 480x640; copy rate %.1f TB/s)\n" % (a.reps, COPY_TBPS))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
