"""The inference drawing on the host (simple_inference.display_on_frame with no_text + the percentile / _viridis depth colouring)
against the device path (planerecnet_amd.render, csrc/prn_render.hip) including its single download, in one process on one seeded
synthetic result.

    timeout -k 10 600 python tools/render_bench.py [--reps 10] [--out profiles/render_bench.txt]

Input: one 480x640 frame, N = 100 and N = 20 instance masks (rectangles and ellipses of 1-12 % of the frame, 5 % holes), boxes around
them, a near-planar depth map.  Prints one JSON line per measurement:
  host     display_on_frame(no_text) + np.percentile x 2 + _viridis, wall clock per frame (the result's tensors are on the device, as the
           model leaves them: the downloads of every mask and of the float frame are part of what the host path does)
  device   render_overlay + colorize_depth + the download of the two uint8 images, wall clock per frame (ends in the blocking copies)
  overlay  the overlay kernel alone: `reps x 10` back-to-back launches between two events, its bytes (N H W mask bytes + 12 H W frame
           bytes + 3 H W output bytes) over that time against the 6.3 TB/s copy rate of the MI355X; with and without outlines
  limits / colours   the same for the five launches of the depth limits and the colouring pass
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
COPY_TBPS = 6.3
H, W = 480, 640


def make_result(N, seed=0):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    masks = np.zeros((N, H, W), bool)
    boxes = np.zeros((N, 4), np.float32)
    for i in range(N):
        h, w = int(H * rng.uniform(0.1, 0.35)), int(W * rng.uniform(0.1, 0.35))
        y0, x0 = rng.randint(0, H - h), rng.randint(0, W - w)
        if i % 2:
            masks[i] = ((yy - y0 - h / 2) / (h / 2)) ** 2 + ((xx - x0 - w / 2) / (w / 2)) ** 2 <= 1
        else:
            masks[i, y0:y0 + h, x0:x0 + w] = True
        boxes[i] = [x0, y0, x0 + w - 1, y0 + h - 1]
    masks &= rng.rand(N, H, W) > 0.05
    depth = (3.0 + 0.002 * xx - 0.001 * yy) * (1 + 0.01 * rng.randn(H, W))
    frame = (rng.rand(H, W, 3) * 255).astype(np.float32)
    result = {"pred_masks": torch.from_numpy(masks).cuda(), "pred_boxes": torch.from_numpy(boxes), "pred_scores": torch.linspace(0.95, 0.3, N).cuda(),
              "pred_depth": torch.from_numpy(depth.astype(np.float32))[None, None].cuda()}
    return result, torch.from_numpy(frame).cuda()


def wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


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


def rate(nbytes, us):
    tbps = nbytes / (us * 1e-6) / 1e12
    return {"us_per_call": round(us, 2), "MB": round(nbytes / 1e6, 2), "effective_TBps": round(tbps, 3), "of_copy_rate": round(tbps / COPY_TBPS, 3)}


def bench(N, reps):
    import simple_inference as si
    from planerecnet_amd import render
    from planerecnet_amd._lib import check, lib
    result, frame = make_result(N)
    lines = []

    def host():
        seg, depth = si.display_on_frame(result, frame, no_text=True)
        return seg, si._viridis(depth, np.percentile(depth, 1), np.percentile(depth, 99))

    def device():
        seg = render.render_overlay(result, frame)
        dep = render.colorize_depth(result["pred_depth"])
        return seg.cpu().numpy(), dep.cpu().numpy()

    h_seg, _ = host()
    d_seg, d_dep = device()
    same = bool(np.array_equal(h_seg, d_seg))
    host_ms, dev_ms = wall(host, max(2, reps // 3), 1), wall(device, reps * 3, 3)
    lines.append({"leg": "host", "N": N, "H": H, "W": W, "ms_per_frame": round(host_ms, 3)})
    depth = result["pred_depth"].squeeze().cpu().numpy()
    lim = render.depth_limits(result["pred_depth"]).cpu().numpy()
    lines.append({"leg": "device", "N": N, "H": H, "W": W, "ms_per_frame": round(dev_ms, 3), "host_over_device": round(host_ms / dev_ms, 1),
                  "overlay_equals_host": same, "limits_equal_numpy": bool(lim[0] == np.percentile(depth, 1) and lim[1] == np.percentile(depth, 99)),
                  "depth_picture_equals_host_at_device_limits": bool(np.array_equal(si._viridis(depth, lim[0], lim[1]).astype(np.uint8), d_dep[:, :, ::-1])),
                  "note": "includes the table uploads, the allocations and the download of the two uint8 images"})
    # the kernels alone, on prepared buffers
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    stream = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))
    m = result["pred_masks"].view(torch.uint8)
    colors = torch.tensor(render.color_table(N), dtype=torch.uint8).cuda()
    boxes = torch.tensor(render.box_table(result["pred_boxes"], N), dtype=torch.int32).cuda()
    out = torch.empty(H, W, 3, dtype=torch.uint8, device="cuda")
    nbytes = N * H * W + 12 * H * W + 3 * H * W
    for layers, what in ((render.LAYER_MASKS | render.LAYER_BOXES, "masks + boxes"), (7, "masks + contours + boxes")):
        us = events(lambda: check(lib.prn_render_overlay(p(frame), p(m), p(colors), p(boxes), N, H, W, 0.5, 0.5, layers, p(out), stream), "overlay"), reps * 10)
        lines.append(dict({"leg": "overlay", "N": N, "layers": what}, **rate(nbytes, us)))
    d = result["pred_depth"].contiguous()
    lim = torch.empty(8, dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.prn_render_limits_ws_bytes(), dtype=torch.uint8, device="cuda")
    us = events(lambda: check(lib.prn_render_depth_limits(p(d), d.numel(), 0.01, 0.99, p(lim), p(ws), stream), "limits"), reps * 10)
    lines.append(dict({"leg": "limits", "launches": 5, "passes_over_the_map": 4}, **rate(4 * 4 * H * W, us)))
    table = torch.tensor(render.viridis_table()[:, ::-1].tolist(), dtype=torch.uint8).cuda()
    dep = torch.empty(H, W, 3, dtype=torch.uint8, device="cuda")
    us = events(lambda: check(lib.prn_render_depth_colors(p(d), d.numel(), p(lim), p(table), p(dep), stream), "colours"), reps * 10)
    lines.append(dict({"leg": "colours"}, **rate(7 * H * W, us)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_bench.py measures on the GPU: none found")
    torch.set_num_threads(4)                                         # as simple_inference.py
    lines = []
    for N in (100, 20):
        for ln in bench(N, a.reps):
            print(json.dumps(ln), flush=True)
            lines.append(ln)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# tools/render_bench.py --reps %d (one MI355X; 480x640)\n" % a.reps)
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
