"""GPU: plane fit and planar depth on the device (csrc/prn_planes.hip through planerecnet_amd.planes) against the reference's
iBims-1 exporter (golden fixture), exact synthetic planes, the fp64 restatement (tests/planes_restate.py) on fuzzed masks, ragged
batches, determinism, no host synchronisation; and the two iBims-1 exporters of simple_inference.py end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from planes_restate import k_of, plane_depth_map, restate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _planes():
    from planerecnet_amd import planes
    return planes


def _near_bound(v, bounds, tol=1e-5):
    """within tol (relative, absolute below 1) of one of the range bounds: where fp32 rounding may decide the NaN rule"""
    return np.any([np.abs(v - b) <= tol * max(1.0, abs(b)) for b in bounds], axis=0)


def _check_against(got, ref, rtol, bounds=None):
    """same NaN pattern (except within 1e-5 of a range bound when `bounds`), relative error <= rtol where both are finite"""
    ng, nr = np.isnan(got), np.isnan(ref)
    if bounds is None:
        assert np.array_equal(ng, nr), int((ng != nr).sum())
    else:
        v = np.where(ng, ref, got).astype(np.float64)
        bad = (ng != nr) & ~_near_bound(v, bounds)
        assert not bad.any(), int(bad.sum())
    f = ~ng & ~nr
    err = np.abs(got[f].astype(np.float64) - ref[f]) / np.maximum(np.abs(ref[f].astype(np.float64)), 1e-30)
    assert err.max(initial=0.0) <= rtol, float(err.max())


def test_device_reproduces_the_reference_exporter(golden_dir):
    z = np.load(os.path.join(golden_dir, "plane_depth.npz"))
    B = z["depth"].shape[0]
    results = [{"pred_depth": torch.from_numpy(z["depth"][b])[None, None].cuda(), "pred_masks": torch.from_numpy(z["masks%d" % b]).cuda()} for b in range(B)]
    single = [_planes().planar_depth([results[b]], z["calib"][b].T, depth_range=(0.0, 10.0))[0] for b in range(B)]
    batched = _planes().planar_depth(results, np.stack([c.T for c in z["calib"]]), depth_range=(0.0, 10.0))
    for b in range(B):
        got = single[b]["pred_plane_depth"]
        assert got.shape == (1, 1) + z["depth"].shape[1:] and got.dtype == torch.float32
        assert torch.equal(got.cpu().isnan(), batched[b]["pred_plane_depth"].cpu().isnan())
        assert torch.equal(got.nan_to_num(0.0), batched[b]["pred_plane_depth"].nan_to_num(0.0))
        _check_against(got.squeeze().cpu().numpy(), z["pred_depths"][b], 1e-6, bounds=(0.0, 10.0))
        assert bool(single[b]["pred_plane_valid"].all())


def test_exact_planes_are_recovered():
    """fp32 depth rendered from known planes n . X = d: the fitted normal within 1e-5 rad, d within 1e-5 relative (one call per image,
    the planes of an image fitted from its own exact depth)"""
    H, W = 96, 128
    K = [k_of(110.0, 100.0, 63.5, 47.5), k_of(90.0, 95.0, 60.0, 50.0)]
    truth = [([0.0, 0.0, 1.0], 3.0), ([0.3, -0.5, 1.0], 2.0), ([-1.0, 0.2, 0.6], 1.2), ([0.0, 1.0, 0.1], 1.4), ([0.2, 0.1, 1.0], 4.0),
             ([0.1, 0.1, -1.0], -2.5)]
    boxes = [(0, 96, 0, 128), (10, 60, 20, 90), (30, 90, 0, 40), (50, 96, 0, 128), (5, 40, 60, 128), (20, 70, 30, 100)]
    for b in range(2):
        for (n, off), (y0, y1, x0, x1) in zip(truth, boxes):
            n = np.asarray(n) / np.linalg.norm(n)
            pd = plane_depth_map(n, off, K[b], H, W)
            m = np.zeros((1, H, W), bool)
            m[0, y0:y1, x0:x1] = True
            m[0] &= pd > 0
            dt = torch.from_numpy(pd.astype(np.float32))[None, None].cuda()
            planes, valid, count = _planes().fit_planes(dt, [torch.from_numpy(m).cuda()], K[b])
            p = planes[0][0].cpu().numpy()
            assert bool(valid[0][0]) and int(count[0][0]) == int(m.sum())
            sign = 1.0 if off >= 0 else -1.0                                          # d >= 0: the normal flips with a negative offset
            ang = np.arccos(min(1.0, float(p[:3] @ n) * sign))
            assert ang <= 1e-5, (b, n, ang)
            assert abs(float(p[3]) - abs(off)) <= 1e-5 * abs(off), (b, n, p[3], off)
            assert abs(np.linalg.norm(p[:3]) - 1.0) <= 1e-12


def _fuzz_image(rng, N, H, W, K):
    """near-planar noisy depth on a noiseless background plane; N masks: random rectangles / ellipses, some on the border, one
    covering the whole image, and degenerate ones (empty, 1 px, 2 px, a 1-pixel line on the planar background)"""
    depth = plane_depth_map([0.05, -0.1, 1.0] / np.linalg.norm([0.05, -0.1, 1.0]), 3.0, K, H, W)
    masks = np.zeros((N, H, W), bool)
    yy, xx = np.mgrid[:H, :W]
    patches = np.zeros((H, W), bool)
    special = {}
    if N >= 7:
        special = {1: "full", 2: "empty", 3: "one", 4: "two", 5: "line", 6: "border"}
    for i in range(N):
        kind = special.get(i, "rect" if rng.rand() < 0.6 else "ellipse")
        if kind == "full":
            masks[i] = True
        elif kind == "empty":
            pass
        elif kind == "one":
            masks[i, rng.randint(H), rng.randint(W)] = True
        elif kind == "two":
            y, x = rng.randint(H), rng.randint(W - 1)
            masks[i, y, x:x + 2] = True
        elif kind == "line":
            y = rng.randint(H)
            masks[i, y, :] = ~patches[y, :]                          # only where the depth is the exact background plane
        else:
            h, w = rng.randint(4, H // 2), rng.randint(4, W // 2)
            y0, x0 = (0, rng.randint(W - w)) if kind == "border" else (rng.randint(H - h + 1), rng.randint(W - w + 1))
            if kind == "ellipse":
                masks[i] = ((yy - y0 - h / 2) / (h / 2)) ** 2 + ((xx - x0 - w / 2) / (w / 2)) ** 2 <= 1
            else:
                masks[i, y0:y0 + h, x0:x0 + w] = True
            if i % 3 == 0:                                            # a noisy tilted patch under this mask
                n = np.array([rng.randn() * 0.4, rng.randn() * 0.4, 1.0])
                pd = plane_depth_map(n / np.linalg.norm(n), 1.5 + 2 * rng.rand(), K, H, W) * (1 + 0.01 * rng.randn(H, W))
                sel = masks[i] & (pd > 0.2) & (pd < 20)
                depth[sel] = pd[sel]
                patches |= sel
            masks[i] &= rng.rand(H, W) > 0.05
    if N >= 7:                                                       # the line must lie on the exact plane: drop it where a patch came later
        masks[5] &= ~patches
    return depth.astype(np.float32), masks


@pytest.mark.parametrize("N,H,W", [(0, 60, 80), (1, 60, 80), (7, 37, 53), (100, 60, 80), (100, 45, 67)])
def test_fuzz_against_the_restatement(N, H, W):
    rng = np.random.RandomState(1000 * N + H)
    K = k_of(70.0 + rng.rand() * 20, 70.0 + rng.rand() * 20, W / 2 - 0.5, H / 2 - 0.5)
    depth, masks = _fuzz_image(rng, N, H, W, K)
    ref, ref_planes, ref_valid = restate(depth, masks, K)
    res = _planes().planar_depth([{"pred_depth": torch.from_numpy(depth)[None, None].cuda(), "pred_masks": torch.from_numpy(masks).cuda()}], K)[0]
    got_valid = res["pred_plane_valid"].cpu()
    assert torch.equal(got_valid, ref_valid), (got_valid.tolist(), ref_valid.tolist())
    if N >= 7:
        assert not got_valid[2:6].any() and bool(got_valid[1])       # empty, 1 px, 2 px, line: invalid; the full-image mask: valid
    gp = res["pred_planes"].cpu()
    v = ref_valid
    assert torch.isnan(gp[~v]).all()
    if v.any():
        assert float((gp[v, :3] * ref_planes[v, :3]).sum(1).min()) >= 1 - 1e-12
        assert float(((gp[v, 3] - ref_planes[v, 3]).abs() / ref_planes[v, 3].abs().clamp_min(1e-6)).max()) <= 1e-9
    _check_against(res["pred_plane_depth"].squeeze().cpu().numpy(), ref, 1e-6)


def test_ragged_batch_is_bit_identical_to_per_image_calls_and_repeats():
    H, W = 60, 80
    rng = np.random.RandomState(7)
    Ks = [k_of(80.0, 82.0, 39.5, 29.5), k_of(75.0, 70.0, 41.0, 28.0), k_of(90.0, 90.0, 40.0, 30.0)]
    imgs = [_fuzz_image(rng, n, H, W, k) for n, k in zip((0, 3, 100), Ks)]
    results = [{"pred_depth": torch.from_numpy(d)[None, None].cuda(), "pred_masks": torch.from_numpy(m).cuda()} for d, m in imgs]
    results[0]["pred_masks"] = None                                  # what the model returns for an image without detections
    kb = torch.from_numpy(np.stack(Ks))
    batched = _planes().planar_depth(results, kb, depth_range=(0.5, 8.0))
    for b in range(3):
        one = _planes().planar_depth([results[b]], Ks[b], depth_range=(0.5, 8.0))[0]
        for key in ("pred_plane_depth", "pred_planes"):
            assert torch.equal(one[key].nan_to_num(123.0), batched[b][key].nan_to_num(123.0)), (b, key)
            assert torch.equal(one[key].isnan(), batched[b][key].isnan())
        assert torch.equal(one["pred_plane_valid"], batched[b]["pred_plane_valid"])
    assert batched[0]["pred_planes"].shape == (0, 4)
    first = torch.cat([r["pred_plane_depth"].flatten() for r in batched]).nan_to_num(123.0)
    planes, valid, count = _planes().fit_planes(torch.cat([r["pred_depth"] for r in results]), [r["pred_masks"] for r in results], kb)
    p0 = torch.cat(planes).nan_to_num(123.0)
    for _ in range(10):
        again = _planes().planar_depth(results, kb, depth_range=(0.5, 8.0))
        assert torch.equal(torch.cat([r["pred_plane_depth"].flatten() for r in again]).nan_to_num(123.0), first)
        pl, va, co = _planes().fit_planes(torch.cat([r["pred_depth"] for r in results]), [r["pred_masks"] for r in results], kb)
        assert torch.equal(torch.cat(pl).nan_to_num(123.0), p0) and torch.equal(torch.cat(va), torch.cat(valid)) and torch.equal(torch.cat(co), torch.cat(count))
    assert [int(c.sum()) for c in count] == [0] + [int(torch.from_numpy(imgs[b][1]).sum()) for b in (1, 2)]


def test_input_is_untouched_and_no_host_synchronisation():
    H, W = 48, 64
    rng = np.random.RandomState(11)
    K = k_of(60.0, 60.0, 31.5, 23.5)
    depth, masks = _fuzz_image(rng, 9, H, W, K)
    results = [{"pred_depth": torch.from_numpy(depth)[None, None].cuda(), "pred_masks": torch.from_numpy(masks).cuda(), "pred_scores": torch.rand(9).cuda()}]
    keep = {k: v.clone() for k, v in results[0].items()}
    k_dev = torch.from_numpy(K).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda").item()                      # the mode does catch a synchronisation
        out = _planes().planar_depth(results, K, depth_range=(0.0, 10.0))
        _planes().fit_planes(results[0]["pred_depth"], [results[0]["pred_masks"]], k_dev)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert set(results[0]) == set(keep)                              # the input dict is not extended ...
    for k, v in keep.items():
        assert torch.equal(results[0][k], v), k                      # ... and its tensors are unchanged
    assert out[0] is not results[0] and out[0]["pred_plane_depth"].data_ptr() != results[0]["pred_depth"].data_ptr()
    assert not torch.equal(out[0]["pred_plane_depth"].nan_to_num(0.0), results[0]["pred_depth"])


def _ibims_inputs(folder, n=2, H=480, W=640):
    sio = pytest.importorskip("scipy.io")
    os.makedirs(folder, exist_ok=True)
    rng = np.random.RandomState(5)
    yy, xx = np.mgrid[:H, :W]
    frames = []
    for s in range(n):
        base = np.stack([128 + 100 * np.sin(xx / (40.0 + 10 * s) + c) * np.cos(yy / (55.0 + 7 * s) - c) for c in (0.0, 1.0, 2.0)], -1)
        rgb = np.clip(base + rng.randn(H, W, 3) * 10, 0, 255).astype(np.uint8)
        K = k_of(518.9 + s, 519.5 - s, 325.6, 253.7)
        sio.savemat(os.path.join(folder, "scene%d.mat" % s), {"data": {"rgb": rgb, "calib": K.T}})
        frames.append((rgb, K))
    return frames


def test_ibims1_exporters_end_to_end(tmp_path):
    sio = pytest.importorskip("scipy.io")
    import simple_inference as si
    from oracle import synth
    from planerecnet_amd.config import cfg, set_cfg
    from planerecnet_amd.planerecnet import PlaneRecNet
    name = "PlaneRecNet_50_config"
    set_cfg(name)
    frames = _ibims_inputs(str(tmp_path / "in"))
    sd = synth.make_state_dict(name, seed=1)
    overrides = {"nms_type": "matrix", "mask_thr": 0.3, "update_thr": 0.3, "top_k": 100}         # what the CLI's defaults put into cfg.solov2
    old = {k: getattr(cfg.solov2, k) for k in overrides}
    old_device = cfg.device
    cfg.solov2.replace(overrides)
    cfg.device = "cuda:0"
    try:
        net = PlaneRecNet(cfg)
        chosen = None
        for shift in (1.0, 2.0, 3.0, 4.0):                                       # condition the category bias: detections must survive
            sd_try = dict(sd)
            sd_try["inst_head.cate_pred.bias"] = sd["inst_head.cate_pred.bias"] + shift
            net.load_state_dict(sd_try)
            net = net.cuda().eval()
            res = [si.ibims1_results(net, rgb) for rgb, _ in frames]
            if all(r["pred_masks"] is not None and r["pred_masks"].shape[0] >= 1 for r in res):
                chosen = sd_try
                break
        assert chosen is not None, "no bias shift leaves a detection"
        ckpt = str(tmp_path / "w.pth")
        torch.save(chosen, ckpt)
        planar = [_planes().planar_depth([r], K, depth_range=(0.0, 10.0))[0] for r, (_, K) in zip(res, frames)]
    finally:
        cfg.solov2.replace(old)
        cfg.device = old_device
    out1, out2 = str(tmp_path / "out1"), str(tmp_path / "out2")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, os.path.join(ROOT, "simple_inference.py"), "--config", name, "--trained_model", ckpt,
           "--ibims1", str(tmp_path / "in") + ":" + out1, "--ibims1_pd", str(tmp_path / "in") + ":" + out2]
    p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    differs = False
    for s, (r, pl) in enumerate(zip(res, planar)):
        for folder in (out1, out2):
            assert os.path.exists(os.path.join(folder, "scene%d_results.png" % s))
        d1 = sio.loadmat(os.path.join(out1, "scene%d_results.mat" % s))["pred_depths"]
        d2 = sio.loadmat(os.path.join(out2, "scene%d_results.mat" % s))["pred_depths"]
        assert d1.dtype == np.float32 and d1.shape == (480, 640) and d2.dtype == np.float32 and d2.shape == (480, 640)
        _check_against(d1, r["pred_depth"].squeeze().cpu().numpy(), 1e-5)
        _check_against(d2, pl["pred_plane_depth"].squeeze().cpu().numpy(), 1e-5, bounds=(0.0, 10.0))
        differs = differs or not np.array_equal(np.nan_to_num(d1, nan=-1.0), np.nan_to_num(d2, nan=-1.0))
    assert differs
