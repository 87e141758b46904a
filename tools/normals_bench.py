"""The normal map of one frame (planerecnet_amd/normals.py; csrc/prn_normals.hip) on the device path against what a user does without it, in
one process on the same seeded inputs:

    timeout -k 10 600 python tools/normals_bench.py [--reps 15] [--out profiles/normals_bench.txt]

Input: the 480 x 640 synthetic room of tools/mesh_bench.py with its labels.  Prints one JSON line per measurement:
  device   `prn_normals` alone on prepared buffers (`event_us.launch`, with labels and the picture; `launch_plain`: no labels, no picture),
           normals.from_depth (`event_us.call`: allocation and intrinsics staging included) -- `reps x 20` back-to-back calls between two
           events after a warm-up -- and the wall clock of one call ending in a synchronise (`call_ms`, median); prn_normal_error of two maps
           the same way (`event_us.error`); `launch_b8`: eight copies of the frame in ONE launch, `per_frame_in_b8` = (launch_b8 - launch) / 7:
           what a frame costs beyond the launch itself
  torch    the same rules written in torch device ops (fp64 points, shifted views); `validity_equal` and `max_abs_diff` say how its output
           compares with the kernel's (a baseline, not a reference: nothing there keeps torch from fusing or reordering)
  numpy    download depth and labels, then the module's own host path; its arrays must equal the device path's bit for bit
  floor    the bytes the rules need moved once -- 4 (+4 with labels) read and 13 (+3 with the picture) written a pixel -- at the HBM rate the
           project's rooflines use (8 TB/s)
All legs are warmed up and measured alternately.  There is no threshold: the baselines of the same run are the yardstick."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK_HBM_GBS = 8000.0                                                # as bench.py


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


def torch_normals(z, lab, k, step=1, gap=0.05):
    """the rules of normals.from_depth (relative gap, same label, camera sign) in torch device ops -> (normals [H,W,3] fp32, valid [H,W])"""
    H, W = z.shape
    fx, fy, cx, cy = (float(x) for x in (k[0, 0], k[1, 1], k[0, 2], k[1, 2]))
    ok = torch.isfinite(z) & (z > 0)
    v, u = torch.meshgrid(torch.arange(H, device=z.device, dtype=torch.float64), torch.arange(W, device=z.device, dtype=torch.float64), indexing="ij")
    z64 = z.double()
    P = torch.stack([(u - cx) * z64 / fx, (v - cy) * z64 / fy, z64], -1)

    def shift(a, dv, du, fill):
        out = torch.full_like(a, fill)
        out[max(0, -dv):H - max(0, dv), max(0, -du):W - max(0, du)] = a[max(0, dv):H + min(0, dv), max(0, du):W + min(0, du)]
        return out

    def neighbour(dv, du):
        zq = shift(z, dv, du, float("nan"))
        zmin = torch.minimum(z, zq)
        use = ok & shift(ok, dv, du, False) & (shift(lab, dv, du, -1) == lab) & ((torch.maximum(z, zq) - zmin) <= gap * zmin)
        return use, shift(P, dv, du, 0.0)

    def tangent(plus, minus):
        (a, pa), (b, pb) = plus, minus
        return torch.where(a[..., None], pa, P) - torch.where(b[..., None], pb, P), a | b

    tu, hu = tangent(neighbour(0, step), neighbour(0, -step))
    tv, hv = tangent(neighbour(step, 0), neighbour(-step, 0))
    n = torch.linalg.cross(tv, tu)
    l2 = (n * n).sum(-1)
    valid = ok & hu & hv & torch.isfinite(l2) & (l2 > 0)
    return torch.where(valid[..., None], n / l2.sqrt()[..., None], torch.zeros_like(n)).float(), valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("normals_bench.py measures on the GPU: none found")
    torch.set_num_threads(4)
    from mesh_bench import room
    from planerecnet_amd import normals as N
    from planerecnet_amd._lib import check, lib
    H, W = 480, 640
    depth, labels, _, K = room(H, W)
    d, l = torch.from_numpy(depth).cuda(), torch.from_numpy(labels).cuda()
    k = torch.from_numpy(K).cuda()
    gap32 = float(np.float32(0.05))
    got = {}

    def device():
        got["device"] = N.from_depth(d, k, l, image=True)

    def torch_ops():
        got["torch"] = torch_normals(d, l, K, gap=gap32)

    def download():
        got["host"] = (d.cpu(), l.cpu())

    def host():
        download()
        got["numpy"] = N.from_depth(got["host"][0], K, got["host"][1], image=True)

    device(), torch_ops(), host()
    n, ok, img = got["device"]
    for x, y, what in zip(got["device"], got["numpy"], ("normals", "valid", "image")):
        assert x.cpu().numpy().tobytes() == y.numpy().tobytes(), "device and numpy %s differ" % what
    validity_equal = bool(torch.equal(got["torch"][1], ok[0]))       # (reported, not asserted: the torch leg is a baseline, not a reference)
    diff = float((got["torch"][0] - n[0]).abs().max())
    t = {"device": [], "torch": [], "numpy": [], "download": []}
    for _ in range(a.reps):                                          # alternating: all see the same machine state
        for name, fn in (("device", device), ("torch", torch_ops), ("numpy", host), ("download", download)):
            fn()                                                     # every timed call follows a call of its own leg
            t[name].append(timed(fn))
    med = {name: float(np.median(v)) for name, v in t.items()}
    us = {"call": events(device, a.reps * 20), "torch": events(torch_ops, a.reps * 4)}
    k9 = k.reshape(1, 9).contiguous()
    okb = ok.view(torch.uint8)
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))

    def launch(lab, image):
        def run():
            check(lib.prn_normals(p(d), p(lab), p(k9), 1, H, W, 1, 0.0, float("inf"), gap32, N.RELATIVE | N.SAME_LABEL, p(n), p(okb), p(image), st), "prn_normals")
        return run
    ref_n, ref_img = n.clone(), img.clone()                          # (the plain launch below overwrites n with the unlabelled map)
    us["launch"] = events(launch(l, img), a.reps * 20)
    us["launch_plain"] = events(launch(None, None), a.reps * 20)
    # a batch of eight copies in one launch: what a frame costs beyond the launch itself is (launch_b8 - launch) / 7
    B8 = 8
    d8, l8, k8 = d.repeat(B8, 1, 1), l.repeat(B8, 1, 1), k9.repeat(B8, 1)
    n8, ok8, img8 = N.from_depth(d8[:, None], k, l8, image=True)
    okb8 = ok8.view(torch.uint8)

    def launch_b8():
        check(lib.prn_normals(p(d8), p(l8), p(k8), B8, H, W, 1, 0.0, float("inf"), gap32, N.RELATIVE | N.SAME_LABEL, p(n8), p(okb8), p(img8), st),
              "prn_normals")
    us["launch_b8"] = events(launch_b8, a.reps * 20)
    assert torch.equal(n8[B8 - 1].view(torch.int32), ref_n[0].view(torch.int32)) and torch.equal(img8[B8 - 1], ref_img[0])
    us["per_frame_in_b8"] = (us["launch_b8"] - us["launch"]) / (B8 - 1)
    launch(l, img)()                                                 # n, valid and the picture hold the labelled map again
    other = N.from_depth(d, k, l, step=3)
    tables = torch.zeros(N.error_bins() + 4, dtype=torch.int64, device="cuda")
    thr = (ctypes.c_double * 3)(*N._thr2((11.25, 22.5, 30), "bench"))
    ob = other[1].view(torch.uint8)

    def error():
        check(lib.prn_normal_error(p(n), p(okb), p(other[0]), p(ob), 1, H * W, thr, 3, p(tables), p(tables[N.error_bins():]), p(tables[N.error_bins() + 3:]), st),
              "prn_normal_error")
    us["error"] = events(error, a.reps * 20)
    nv = int(ok.sum())
    moved, moved_plain = H * W * (4 + 4 + 13 + 3), H * W * (4 + 13)
    floor_us, floor_plain_us = moved / (PEAK_HBM_GBS * 1e9) * 1e6, moved_plain / (PEAK_HBM_GBS * 1e9) * 1e6
    tag = {"size": "%dx%d" % (H, W), "normals": nv, "reps": a.reps}
    lines = [dict(tag, leg="device", event_us={name: round(v, 2) for name, v in us.items() if name != "torch"}, call_ms=round(med["device"], 4),
                  call_min_ms=round(min(t["device"]), 4), block_pixels=N.block_pixels(), arrays_equal_numpy=True),
             dict(tag, leg="torch", event_us=round(us["torch"], 1), call_ms=round(med["torch"], 3), max_abs_diff=diff, validity_equal=validity_equal,
                  torch_over_device_call=round(med["torch"] / med["device"], 1)),
             dict(tag, leg="numpy", ms=round(med["numpy"], 3), min_ms=round(min(t["numpy"]), 3), download_ms=round(med["download"], 3),
                  downloaded_MB=round(H * W * 8 / 1e6, 2), numpy_over_device_call=round(med["numpy"] / med["device"], 1)),
             dict(tag, leg="floor", moved_MB=round(moved / 1e6, 2), hbm_GBs=PEAK_HBM_GBS, floor_us=round(floor_us, 2), launch_over_floor=round(us["launch"] / floor_us, 1),
                  achieved_GBs=round(moved / (us["launch"] * 1e-6) / 1e9, 1), plain_moved_MB=round(moved_plain / 1e6, 2), plain_floor_us=round(floor_plain_us, 2),
                  plain_launch_over_floor=round(us["launch_plain"] / floor_plain_us, 1))]
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# tools/normals_bench.py --reps %d (one MI355X)\n" % a.reps)
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
