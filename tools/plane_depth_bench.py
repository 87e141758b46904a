"""Plane fit + planar depth (planerecnet_amd.planes, csrc/prn_planes.hip) against the reference's per-instance torch loop on the GPU.

    timeout -k 10 900 python tools/plane_depth_bench.py [--reps 20] [--rocprof]

Input: B = 1 and 8 images of 480x640, N = 100 instance masks each (rectangles and ellipses of 1-12 % of the frame, 5 % holes),
near-planar depth.  Prints one JSON line per measurement:
  device   fit + render per call (CUDA events around `reps` calls), effective bandwidth (mask + depth bytes) / time against the
           measured 6.3 TB/s copy rate of the MI355X
  loop     the reference's exporter loop (simple_inference.py:268-301: boolean indexing, torch.svd, torch.where per instance) on the
           same input, per image (B = 1 only: it is N host round trips per image)
--rocprof  additionally runs the device leg as a child under `rocprofv3 --kernel-trace --stats` and reports each of the three
           kernels' average duration and the moments pass's effective bandwidth."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TBPS = 6.3
H, W, N = 480, 640, 100


def make_input(B, seed=0):
    rng = np.random.RandomState(seed)
    K = np.array([[518.9, 0.0, 325.6], [0.0, 519.5, 253.7], [0.0, 0.0, 1.0]])
    yy, xx = np.mgrid[:H, :W]
    depth = np.empty((B, 1, H, W), np.float32)
    masks = np.zeros((B, N, H, W), bool)
    for b in range(B):
        r = (np.linalg.inv(K) @ np.stack([xx.ravel(), yy.ravel(), np.ones(H * W)])).reshape(3, H, W)
        n = np.array([0.05, -0.1, 1.0])
        depth[b, 0] = 3.0 / np.einsum("i,ihw->hw", n, r) * (1 + 0.01 * rng.randn(H, W))
        for i in range(N):
            h, w = int(H * rng.uniform(0.1, 0.35)), int(W * rng.uniform(0.1, 0.35))
            y0, x0 = rng.randint(0, H - h), rng.randint(0, W - w)
            if i % 2:
                masks[b, i] = ((yy - y0 - h / 2) / (h / 2)) ** 2 + ((xx - x0 - w / 2) / (w / 2)) ** 2 <= 1
            else:
                masks[b, i, y0:y0 + h, x0:x0 + w] = True
        masks[b] &= rng.rand(N, H, W) > 0.05
    return torch.from_numpy(depth).cuda(), [torch.from_numpy(masks[b]).cuda() for b in range(B)], K


def time_device(B, reps, warmup=3):
    from planerecnet_amd import planes
    depth, masks, K = make_input(B)
    results = [{"pred_depth": depth[b:b + 1], "pred_masks": masks[b]} for b in range(B)]
    for _ in range(warmup):
        planes.planar_depth(results, K, depth_range=(0.0, 10.0))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        planes.planar_depth(results, K, depth_range=(0.0, 10.0))
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    nbytes = B * N * H * W + B * H * W * 4
    return {"leg": "device", "B": B, "N": N, "H": H, "W": W, "ms_per_call": round(ms, 4), "input_MB": round(nbytes / 1e6, 2),
            "effective_TBps": round(nbytes / (ms * 1e-3) / 1e12, 3), "of_copy_rate": round(nbytes / (ms * 1e-3) / 1e12 / COPY_TBPS, 3),
            "note": "event-timed, includes the host-side launch path of planar_depth (table uploads, allocations)"}


def reference_loop(pred_depth, pred_masks, k_matrix):
    """simple_inference.py:268-301 of the reference, as it runs there (one image)"""
    k_matrix = torch.from_numpy(k_matrix).double().cuda()
    intrinsic_inv = torch.inverse(k_matrix).double().cuda()
    _, _, h, w = pred_depth.shape
    cx, cy, fx, fy = k_matrix[0][2], k_matrix[1][2], k_matrix[0][0], k_matrix[1][1]
    v, u = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    Z = pred_depth.squeeze(dim=0)
    point_cloud = torch.cat(((u - cx) * Z / fx, (v - cy) * Z / fy, Z), dim=0).permute(1, 2, 0)
    x = torch.arange(w, dtype=torch.float32).view(1, w).repeat(h, 1)
    y = torch.arange(h, dtype=torch.float32).view(h, 1).repeat(1, w)
    xy1 = torch.stack((x, y, torch.ones((h, w)))).view(3, -1).double().cuda()
    k_inv_dot_xy1 = torch.matmul(intrinsic_inv.squeeze(), xy1)
    plane_depths = []
    for idx in range(pred_masks.shape[0]):
        pts = point_cloud[pred_masks[idx].bool(), :].squeeze(dim=0)
        mean = pts.mean(dim=0)
        adj = pts - mean
        U, _, _ = torch.svd(torch.mm(adj.transpose(0, 1), adj))
        normal = U[:, 2]
        plane_depths.append(torch.dot(mean, normal) / torch.matmul(normal, k_inv_dot_xy1))
    plane_depths = torch.stack(plane_depths, dim=0).view(-1, h, w)
    out = pred_depth.squeeze()
    for i in range(plane_depths.shape[0]):
        out = torch.where(pred_masks[i], plane_depths[i].float(), out)
    out = out.cpu().numpy()
    out[out <= 0] = np.nan
    out[out >= 10] = np.nan
    return out


def time_loop(reps=3):
    depth, masks, K = make_input(1)
    reference_loop(depth, masks[0], K)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        reference_loop(depth, masks[0], K)
    torch.cuda.synchronize()
    return {"leg": "loop", "B": 1, "N": N, "H": H, "W": W, "ms_per_image": round((time.perf_counter() - t0) / reps * 1e3, 3)}


def rocprof(B, reps):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "planes", "--",
               sys.executable, os.path.abspath(__file__), "--inner", str(B), "--reps", str(reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise RuntimeError("rocprofv3 run failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel statistics")
        rows = list(csv.DictReader(open(files[0])))
    out = {"leg": "rocprof", "B": B, "N": N, "H": H, "W": W}
    nbytes = B * N * H * W + B * H * W * 4
    total = 0.0
    for key in ("planes_moments_kernel", "planes_solve_kernel", "planes_render_kernel"):
        r = [q for q in rows if key in q["Name"]]
        if not r:
            continue
        avg_us = float(r[0]["AverageNs"]) / 1e3
        total += avg_us
        out[key + "_us"] = round(avg_us, 2)
    if "planes_moments_kernel_us" in out:
        bw = nbytes / (out["planes_moments_kernel_us"] * 1e-6) / 1e12
        out["moments_effective_TBps"] = round(bw, 3)
        out["moments_of_copy_rate"] = round(bw / COPY_TBPS, 3)
    out["three_kernels_us"] = round(total, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--inner", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    torch.set_num_threads(4)
    if a.inner:
        time_device(a.inner, a.reps)
        return
    for B in (1, 8):
        print(json.dumps(time_device(B, a.reps)), flush=True)
    if not a.no_loop:
        loop = time_loop()
        print(json.dumps(loop), flush=True)
    if a.rocprof:
        for B in (1, 8):
            r = rocprof(B, a.reps)
            if B == 1 and not a.no_loop:
                r["loop_over_three_kernels"] = round(loop["ms_per_image"] * 1e3 / r["three_kernels_us"], 1)
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
