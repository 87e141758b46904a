"""The overlap tables of one frame -- what every plane-level evaluation figure is computed from (planerecnet_amd/plane_eval.py;
csrc/prn_plane_eval.hip) -- on the device path against the two things a user does without it, alternating in one process on the same seeded
inputs:

    timeout -k 10 900 python tools/plane_eval_bench.py [--reps 7] [--out profiles/plane_eval_bench.txt]

Input: one 480 x 640 frame, A = 20 ground-truth planes and B = 100 detections (overlapping ellipses with holes), two depth maps.  Prints one
JSON line per measurement:
  device    two label_map calls and one overlap call (the work of PlaneEvalAccumulator.add_frame); wall clock ending in a synchronise;
            `after_80ms_idle_ms` is the same call after the process slept 80 ms with the device idle (the time of one host-side leg)
  dense     the published formulation in torch operations on the device: [A+1,1,HW] * [1,c,HW] float masks summed over the pixels, the
            detections in chunks of `--chunk` so that the temporaries fit; counts and per-pair error sums in fp32 -- its counts must equal the
            device path's, its sums are compared loosely (fp32 against integers)
  bincount  download both mask sets and both depth maps, paint by argmax, numpy.bincount; tables must equal the device path's bit for bit
  paint_call  label_map of the B detections as one tensor (prn_label_map_flat: nothing uploaded) and as a list of two images (prn_label_map: two
            small tables through pinned memory), alternating
  kernels   the launches alone, `reps x 20` back-to-back calls between two events on prepared buffers: the paint of the B detections, and
            the table kernel on (a) the frame's maps, (b) every pixel in one bin -- every run of every thread of a workgroup adds to one LDS
            address, (c) a checkerboard -- every run is one pixel long, (d) the frame's maps through the global-atomics path (the same maps,
            table dimensions above the LDS limit)
All legs are warmed up and measured alternately, every timed call directly after an untimed call of the same leg.  There is no threshold: the baselines of the same run are the yardstick."""
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


def ellipses(seed, n, H, W):
    """n masks: a filled ellipse each with a few pin-holes; they overlap"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((n, H, W), bool)
    for i in range(n):
        cy, cx = rng.uniform(0.1, 0.9) * H, rng.uniform(0.1, 0.9) * W
        ry, rx = rng.uniform(0.05, 0.3) * H + 1, rng.uniform(0.05, 0.3) * W + 1
        out[i] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0) & (rng.rand(H, W) > 0.01)
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


def dense_tables(gt, pred, gt_depth, pred_depth, chunk):
    """the broadcast formulation on the device: -> (count, error sum) fp32 [A+1, B+1], row / column 0 = the complement of the masks"""
    A, B = gt.shape[0], pred.shape[0]
    HW = gt.shape[1] * gt.shape[2]

    def exclusive(m):                                                # first mask wins, then the complement in front
        m = m.reshape(m.shape[0], HW)
        claimed = torch.cumsum(m.int(), 0) - m.int()
        own = m & (claimed == 0)
        return torch.cat([~m.any(0, keepdim=True), own]).float()
    g, p = exclusive(gt), exclusive(pred)
    err = (pred_depth.reshape(HW) - gt_depth.reshape(HW)).abs()
    err = torch.where(gt_depth.reshape(HW) < 1e-4, torch.zeros_like(err), err).clamp(max=1024.0)
    count, esum = torch.empty(A + 1, B + 1, device=gt.device), torch.empty(A + 1, B + 1, device=gt.device)
    for c0 in range(0, B + 1, chunk):
        both = g[:, None, :] * p[None, c0:c0 + chunk, :]             # [A+1, c, HW] float
        count[:, c0:c0 + chunk] = both.sum(2)
        esum[:, c0:c0 + chunk] = (both * err).sum(2)
    return count, esum


def bincount_tables(gt, pred, gt_depth, pred_depth):
    """download, paint by argmax, numpy.bincount -> (T, S) int64"""
    from planerecnet_amd.plane_eval import _label_map_np, _overlap_np
    g, p = gt.cpu().numpy(), pred.cpu().numpy()
    da, db = gt_depth.cpu().numpy(), pred_depth.cpu().numpy()
    la, lb = _label_map_np(g, False), _label_map_np(p, False)
    T, S = _overlap_np(la[None], lb[None], g.shape[0], p.shape[0], da[None], db[None])
    return T[0], S[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=8, help="detections per chunk of the dense formulation")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plane_eval_bench.py measures on the GPU: none found")
    torch.set_num_threads(4)                                         # as eval.py
    from planerecnet_amd import plane_eval as P
    from planerecnet_amd._lib import check, lib
    H, W, A, B = 480, 640, 20, 100
    gt, pred = torch.from_numpy(ellipses(1, A, H, W)).cuda(), torch.from_numpy(ellipses(2, B, H, W)).cuda()
    rng = np.random.RandomState(3)
    gd = (0.5 + 4.0 * rng.rand(H, W)).astype(np.float32)
    gd[rng.rand(H, W) < 0.1] = 0.0
    gt_depth = torch.from_numpy(gd).cuda()
    pred_depth = torch.from_numpy((gd + 0.2 * rng.randn(H, W)).astype(np.float32)).cuda()

    def device():
        return P.overlap(P.label_map(gt), P.label_map(pred), A, B, gt_depth, pred_depth)

    def dense():
        return dense_tables(gt, pred, gt_depth, pred_depth, a.chunk)

    def bincount():
        return bincount_tables(gt, pred, gt_depth, pred_depth)

    (T, S), (dc, ds), (bt, bs) = device(), dense(), bincount()
    T, S = T.cpu().numpy(), S.cpu().numpy()
    assert np.array_equal(T, bt) and np.array_equal(S, bs), "device and bincount tables differ"
    assert np.array_equal(dc.cpu().numpy().astype(np.int64), T), "device and dense counts differ"
    dense_rel = float(np.abs(ds.double().cpu().numpy() * P.DEPTH_SCALE - S).max() / max(S.max(), 1))
    for _ in range(2):
        device(), dense(), bincount()
    t = {"device": [], "dense": [], "bincount": [], "idle": []}
    for _ in range(a.reps):                                          # alternating: all see the same machine state
        for name, fn in (("device", device), ("dense", dense), ("bincount", bincount)):
            fn()                                                     # every timed call follows a call of its own leg: frames come back to back
            t[name].append(timed(fn))
        torch.cuda.synchronize()
        time.sleep(0.08)                                             # ... and what a call costs after the device sat idle for a host-side leg's time
        t["idle"].append(timed(device))
    med = {k: float(np.median(v)) for k, v in t.items()}
    tag = {"size": "%dx%d" % (H, W), "A": A, "B": B, "reps": a.reps}
    lines = [dict(tag, leg="device", ms=round(med["device"], 4), min_ms=round(min(t["device"]), 4), after_80ms_idle_ms=round(med["idle"], 4), after_80ms_idle_min_max_ms=[round(min(t["idle"]), 3), round(max(t["idle"]), 3)], tables_equal=True,
                  bins=(A + 1) * (B + 1), nonzero_bins=int((T > 0).sum())),
             dict(tag, leg="dense", ms=round(med["dense"], 3), min_ms=round(min(t["dense"]), 3), chunk=a.chunk,
                  temporaries_MB=round(2 * (A + 1) * min(a.chunk, B + 1) * H * W * 4 / 1e6, 1), whole_MB=round((A + 1) * (B + 1) * H * W * 4 / 1e6, 1),
                  counts_equal=True, sum_rel_err=float("%.2e" % dense_rel), dense_over_device=round(med["dense"] / med["device"], 1)),
             dict(tag, leg="bincount", ms=round(med["bincount"], 3), min_ms=round(min(t["bincount"]), 3), downloaded_MB=round(((A + B) * H * W + 8 * H * W) / 1e6, 1),
                  bincount_over_device=round(med["bincount"] / med["device"], 1))]
    # what the pointer table of a list costs: the paint of the B detections as a single tensor (no upload) and as a list of two images
    calls = {"tensor": [], "list": []}
    for _ in range(a.reps):
        for name, fn in (("tensor", lambda: P.label_map(pred)), ("list", lambda: P.label_map([pred, None]))):
            fn()
            calls[name].append(timed(fn))
    lines.append(dict(tag, leg="paint_call", tensor_ms=round(float(np.median(calls["tensor"])), 4), list_of_two_ms=round(float(np.median(calls["list"])), 4)))
    # the launches alone, on prepared buffers
    p = lambda x: ctypes.c_void_p(x.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))
    pred8 = pred.view(torch.uint8)
    ptrs = torch.tensor([pred8.data_ptr()], dtype=torch.int64).cuda()
    first = torch.tensor([0, B], dtype=torch.int32).cuda()
    labels = torch.empty(H, W, dtype=torch.int32, device="cuda")
    la, lb = P.label_map(gt), P.label_map(pred)
    yy, xx = np.mgrid[:H, :W]
    board = torch.from_numpy((1 + (yy + xx) % 2).astype(np.int32)).cuda()
    one = torch.ones(H, W, dtype=torch.int32, device="cuda")
    tables = torch.zeros(2, 64 * 101, dtype=torch.int64, device="cuda")

    def paint():
        check(lib.prn_label_map(p(ptrs), p(first), 1, H, W, 0, p(labels), st), "prn_label_map")

    def table(x, y, na, nb):
        def run():
            check(lib.prn_label_overlap(p(x), p(y), p(gt_depth), p(pred_depth), 1, H, W, na, nb, p(tables[0]), p(tables[1]), st), "prn_label_overlap")
        return run

    us = {"paint_%d_masks" % B: events(paint, a.reps * 20)}
    assert torch.equal(labels, lb)
    for name, fn in (("frame_lds", table(la, lb, A, B)), ("one_bin_lds", table(one, one, A, B)), ("checkerboard_lds", table(board, board, A, B)),
                     ("frame_global", table(la, lb, 63, B)), ("one_bin_global", table(one, one, 63, B)), ("checkerboard_global", table(board, board, 63, B))):
        us[name] = events(fn, a.reps * 20)
    lines.append(dict(tag, leg="kernels", us={k: round(v, 2) for k, v in us.items()}, mask_MB=round(B * H * W / 1e6, 2), maps_and_depths_MB=round(16 * H * W / 1e6, 2),
                      lds_bins=P.LDS_BINS, global_path_bins=64 * (B + 1)))
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# tools/plane_eval_bench.py --reps %d --chunk %d (one MI355X)\n" % (a.reps, a.chunk))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
