"""Robust plane fit (planes.fit_planes_ransac, csrc/prn_planes_ransac.hip) against its floor and against what a user would write today.

    timeout -k 10 900 python tools/plane_ransac_bench.py [--reps 20] [--rocprof] [--out FILE]

Input: tools/plane_depth_bench.py's -- B = 1 and 8 images of 480x640, N = 100 instance masks each, near-planar depth.  One JSON line per
measurement (also appended to --out):
  ransac   fit_planes_ransac (threshold 0.05 m, 256 hypotheses, one refinement) per call, device events around `reps` calls after a warm-up;
           `tests`: mask pixels x hypotheses (what the algorithm needs), `issued`: pixels of the non-empty (64 x 16 pixel block, instance) pairs x
           hypotheses (what the score kernel executes)
  lsq      fit_planes on the same input: the floor, one pass over the masks
  torch    the same algorithm per instance in torch operations on the device (boolean indexing, a [pixels, hypotheses] residual matrix, argmax,
           torch.linalg.eigh for the refits), B = 1: N host round trips per image
--rocprof  additionally runs the ransac leg as a child under `rocprofv3 --kernel-trace --stats` (a run of its own) and reports every kernel's
           average duration and the score kernel's point-plane tests per second (needed and issued)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from plane_depth_bench import H, N, W, make_input      # noqa: E402

OPTS = {"threshold": 0.05, "relative": False, "hypotheses": 256, "refine": 1, "seed": 0}
KERNELS = ("ransac_count_kernel", "ransac_scan_kernel", "ransac_sample_kernel", "ransac_score_kernel", "ransac_select_kernel", "ransac_classify_kernel",
           "planes_moments_kernel", "planes_solve_kernel", "ransac_finish_kernel")


def work(masks):
    """(needed, issued) point-plane tests of the score kernel for a list of [N,H,W] bool masks"""
    needed = issued = 0
    for m in masks:
        flat = m.reshape(m.shape[0], -1)
        needed += int(flat.sum()) * OPTS["hypotheses"]
        n, h, w = m.shape
        blocks = torch.nn.functional.pad(m, (0, (-w) % 64, 0, (-h) % 16)).reshape(n, (h + 15) // 16, 16, (w + 63) // 64, 64).any(4).any(2)
        issued += int(blocks.sum()) * 1024 * OPTS["hypotheses"]
    return needed, issued


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def time_device(B, reps):
    from planerecnet_amd import planes
    depth, masks, K = make_input(B)
    needed, issued = work(masks)
    out = []
    ms = timed(lambda: planes.fit_planes_ransac(depth, masks, K, **OPTS), reps)
    out.append({"leg": "ransac", "B": B, "N": N, "H": H, "W": W, **OPTS, "ms_per_call": round(ms, 4), "tests": needed, "issued": issued,
                "note": "event-timed, includes the host-side launch path (table uploads, allocations)"})
    ms = timed(lambda: planes.fit_planes(depth, masks, K), reps)
    out.append({"leg": "lsq", "B": B, "N": N, "H": H, "W": W, "ms_per_call": round(ms, 4)})
    return out


def torch_ransac(depth, masks, k_matrix, threshold, hypotheses, refine, generator):
    """one image: the contract's algorithm with torch operations per instance (torch's generator instead of Philox)"""
    k = torch.as_tensor(k_matrix, dtype=torch.float64, device=depth.device)
    h, w = depth.shape[-2:]
    v, u = torch.meshgrid(torch.arange(h, device=depth.device), torch.arange(w, device=depth.device), indexing="ij")
    Z = depth.reshape(h, w).double()
    cloud = torch.stack(((u - k[0, 2]) * Z / k[0, 0], (v - k[1, 2]) * Z / k[1, 1], Z), -1)

    def lsq(pts):
        if pts.shape[0] < 3:
            return None
        c = pts.mean(0)
        adj = pts - c
        evals, evecs = torch.linalg.eigh(adj.T @ adj)
        if not bool(evals[1] > 1e-12 * evals[2]):
            return None
        n = evecs[:, 0]
        d = torch.dot(c, n)
        return torch.cat([n, d[None]]) * (-1.0 if d < 0 else 1.0)

    planes = []
    for i in range(masks.shape[0]):
        pts = cloud[masks[i]]
        plane = None
        if pts.shape[0] >= 3:
            p = pts[torch.randint(pts.shape[0], (hypotheses, 3), device=pts.device, generator=generator)]
            e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
            c = torch.linalg.cross(e1, e2)
            cc = (c * c).sum(1)
            ok = cc > 1e-12 * (e1 * e1).sum(1) * (e2 * e2).sum(1)
            n = c / cc.sqrt()[:, None]
            d = (n * p[:, 0]).sum(1)
            inl = ((pts @ n.T - d).abs() <= threshold) & ok
            score = inl.sum(0)
            best = int(score.argmax())
            if int(score[best]) >= 3:
                plane = lsq(pts[inl[:, best]])
                for _ in range(refine):
                    if plane is None:
                        break
                    plane = lsq(pts[(pts @ plane[:3] - plane[3]).abs() <= threshold])
        planes.append(plane)
    return planes


def time_torch(reps=3):
    depth, masks, K = make_input(1)
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    run = lambda: torch_ransac(depth[0], masks[0], K, OPTS["threshold"], OPTS["hypotheses"], OPTS["refine"], g)      # noqa: E731
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    return {"leg": "torch", "B": 1, "N": N, "H": H, "W": W, "ms_per_image": round((time.perf_counter() - t0) / reps * 1e3, 3)}


def rocprof(B, reps):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "ransac", "--",
               sys.executable, os.path.abspath(__file__), "--inner", str(B), "--reps", str(reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise RuntimeError("rocprofv3 run failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel statistics")
        rows = list(csv.DictReader(open(files[0])))
    _, masks, _ = make_input(B)
    needed, issued = work(masks)
    out = {"leg": "rocprof", "B": B, "N": N, "H": H, "W": W, "hypotheses": OPTS["hypotheses"], "refine": OPTS["refine"]}
    total = 0.0
    for key in KERNELS:
        r = [q for q in rows if key in q["Name"]]
        if not r:
            continue
        avg_us = sum(float(q["AverageNs"]) * int(q["Calls"]) for q in r) / sum(int(q["Calls"]) for q in r) / 1e3
        per_call = sum(int(q["Calls"]) for q in r) / (reps + 3)                                   # launches per fit_planes_ransac call
        out[key + "_us"] = round(avg_us, 2)
        out[key + "_launches"] = round(per_call, 2)
        total += avg_us * per_call
    if "ransac_score_kernel_us" in out:
        out["score_Gtests_per_s"] = round(needed / out["ransac_score_kernel_us"] / 1e3, 1)
        out["score_issued_Gtests_per_s"] = round(issued / out["ransac_score_kernel_us"] / 1e3, 1)
    out["kernels_us_per_call"] = round(total, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--inner", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plane_ransac_bench.py measures on the GPU: no device found")
    torch.set_num_threads(4)
    if a.inner:
        from planerecnet_amd import planes
        depth, masks, K = make_input(a.inner)
        timed(lambda: planes.fit_planes_ransac(depth, masks, K, **OPTS), a.reps)
        return

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    for B in (1, 8):
        for rec in time_device(B, a.reps):
            emit(rec)
    if not a.no_torch:
        emit(time_torch())
    if a.rocprof:
        for B in (1, 8):
            emit(rocprof(B, a.reps))


if __name__ == "__main__":
    main()
