"""The mesh of one frame (planerecnet_amd/reconstruct.py; csrc/prn_mesh.hip) on the device path against what a user does without it, in one
process on the same seeded inputs:

    timeout -k 10 600 python tools/mesh_bench.py [--reps 15] [--out profiles/mesh_bench.txt]

Input: one 480 x 640 frame of a synthetic room -- a floor, a slanted wall and a box, each with its label, about 1 % of the pixels NaN / inf /
zero / negative -- with colours.  Prints one JSON line per measurement:
  device   reconstruct.mesh (four launches) and reconstruct.point_cloud (three): `reps x 20` back-to-back calls between two events after a
           warm-up (`event_us`; `*_launches`: the library call alone on prepared buffers, no allocation), and the wall clock of one call
           ending in a synchronise (`call_ms`, median; allocation of the outputs included)
  numpy    download depth, labels and colours, then the same arrays with vectorised numpy (the module's own host path); its arrays must
           equal the device path's bit for bit.  `download_ms` is the transfer alone
  floor    the bytes the rules need moved once -- 15 bytes a pixel in and out (depth, label, colour; the id map), 19 a vertex, 12 a face -- at
           the HBM rate the project's rooflines use (8 TB/s): a lower bound no implementation of four dependent launches reaches
All legs are warmed up and measured alternately.  There is no threshold: the baselines of the same run are the yardstick."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM_GBS = 8000.0                                                # as bench.py


def room(H, W, seed=0, holes=0.01):
    """-> (depth float32 [H,W], labels int32 [H,W], colors uint8 [H,W,3], K float64 [3,3])"""
    rng = np.random.RandomState(seed)
    K = np.array([[518.9, 0.0, 325.6], [0.0, 519.5, 253.7], [0.0, 0.0, 1.0]])
    v, u = np.mgrid[:H, :W].astype(np.float64)
    rx, ry = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    with np.errstate(all="ignore"):
        floor = np.where(ry > 1e-3, 1.2 / ry, np.inf)
    wall = 4.0 / (1.0 + 0.3 * rx)
    depth, labels = np.minimum(floor, wall), np.where(floor < wall, 1, 2)
    box = (np.abs(rx + 0.1) < 0.18) & (np.abs(ry - 0.1) < 0.15)
    depth, labels = np.where(box, 2.0 + 0.1 * rx, depth).astype(np.float32), np.where(box, 3, labels).astype(np.int32)
    bad = rng.rand(H, W) < holes
    depth[bad] = rng.choice(np.array([np.nan, np.inf, 0.0, -1.0], dtype=np.float32), size=int(bad.sum()))
    return depth, labels, rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8), K


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench.py measures on the GPU: none found")
    torch.set_num_threads(4)
    from planerecnet_amd import reconstruct as rc
    H, W = 480, 640
    depth, labels, colors, K = room(H, W)
    d, l, c = (torch.from_numpy(x).cuda() for x in (depth, labels, colors))
    k = torch.from_numpy(K).cuda()
    got = {}

    def device():
        got["mesh"] = rc.mesh(d, k, l, c)

    def cloud():
        got["cloud"] = rc.point_cloud(d, k, l, c)

    def download():
        got["host"] = (d.cpu(), l.cpu(), c.cpu())

    def host():
        download()
        got["numpy"] = rc.mesh(got["host"][0], K, got["host"][1], got["host"][2])

    device(), cloud(), host()
    dm, hm = got["mesh"].cpu()[0], got["numpy"].cpu()[0]
    for key in ("vertices", "faces", "labels", "colors"):
        assert dm[key].tobytes() == hm[key].tobytes(), "device and numpy %s differ" % key
    nv, nf = (int(x) for x in got["mesh"].counts[0].tolist())
    t = {"device": [], "cloud": [], "numpy": [], "download": []}
    for _ in range(a.reps):                                          # alternating: all see the same machine state
        for name, fn in (("device", device), ("cloud", cloud), ("numpy", host), ("download", download)):
            fn()                                                     # every timed call follows a call of its own leg
            t[name].append(timed(fn))
    med = {n: float(np.median(v)) for n, v in t.items()}
    us = {"mesh": events(device, a.reps * 20), "point_cloud": events(cloud, a.reps * 20)}
    # the launches alone: the library call on prepared buffers (no allocation, no intrinsics staging)
    import ctypes
    from planerecnet_amd._lib import check, lib
    m = got["mesh"]
    k9 = k.reshape(1, 9).contiguous()
    ws = torch.empty(lib.prn_mesh_ws_bytes(1, H, W) // 4, dtype=torch.int32, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))

    def launches(flags):
        def run():
            check(lib.prn_mesh(p(d), p(l), p(c), p(k9), 1, H, W, 0.0, float("inf"), 0.05, flags, p(ws), p(m.vertices), p(m.labels), p(m.colors), p(m.vertex_id),
                               p(m.faces), p(m.counts), st), "prn_mesh")
        return run
    us["mesh_launches"] = events(launches(rc.RELATIVE | rc.SAME_LABEL | rc.FACES), a.reps * 20)
    us["point_cloud_launches"] = events(launches(rc.RELATIVE | rc.SAME_LABEL), a.reps * 20)
    again = rc.Mesh(m.vertices, m.labels, m.colors, m.faces, m.counts, m.vertex_id).cpu()[0]          # (the last call wrote no faces: counts say so)
    assert again["vertices"].tobytes() == hm["vertices"].tobytes() and again["faces"].shape[0] == 0
    moved = H * W * 15 + nv * 19 + nf * 12
    floor_us = moved / (PEAK_HBM_GBS * 1e9) * 1e6
    tag = {"size": "%dx%d" % (H, W), "vertices": nv, "faces": nf, "reps": a.reps}
    lines = [dict(tag, leg="device", event_us={n: round(v, 2) for n, v in us.items()}, call_ms=round(med["device"], 4), call_min_ms=round(min(t["device"]), 4),
                  point_cloud_call_ms=round(med["cloud"], 4), block_pixels=rc.block_pixels(), scan_chunk=rc.scan_chunk(), arrays_equal_numpy=True),
             dict(tag, leg="numpy", ms=round(med["numpy"], 3), min_ms=round(min(t["numpy"]), 3), download_ms=round(med["download"], 3),
                  downloaded_MB=round(H * W * 11 / 1e6, 2), numpy_over_device_call=round(med["numpy"] / med["device"], 1)),
             dict(tag, leg="floor", moved_MB=round(moved / 1e6, 2), hbm_GBs=PEAK_HBM_GBS, floor_us=round(floor_us, 2),
                  launches_over_floor=round(us["mesh_launches"] / floor_us, 1), achieved_GBs=round(moved / (us["mesh_launches"] * 1e-6) / 1e9, 1))]
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# tools/mesh_bench.py --reps %d (one MI355X)\n" % a.reps)
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
