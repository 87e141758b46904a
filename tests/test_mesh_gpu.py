"""GPU: the mesh of a depth map on the device (csrc/prn_mesh.hip through planerecnet_amd.reconstruct) against the numpy restatement
(tests/mesh_restate.py), exactly -- vertices, labels, colours, faces, counts and the id map compared as bits -- at sizes that straddle every
launch-shape branch (read from the library's exported constants), over validity patterns, batches, the point cloud, determinism, untouched
inputs, no host synchronisation, library refusals with real buffers, reconstruct_results over planes.planar_depth, and `--ibims1_pd --ply`
of simple_inference.py end to end."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rc():
    from planerecnet_amd import reconstruct
    return reconstruct


def _dev(depth, labels=None, colors=None):
    return (torch.from_numpy(np.ascontiguousarray(depth)).cuda(), None if labels is None else torch.from_numpy(np.ascontiguousarray(labels)).cuda(),
            None if colors is None else torch.from_numpy(np.ascontiguousarray(colors)).cuda())


def _check(depth, K, labels=None, colors=None, **kw):
    """one image on the device == the restatement, bit for bit; -> the restatement's dict"""
    d, l, c = _dev(depth, labels, colors)
    got = R.from_mesh(_rc().mesh(d, K, l, c, **kw))[0]
    want = R.mesh_vec(depth, K, labels, colors, **kw)
    assert got["counts"] == want["counts"], (depth.shape, kw, got["counts"], want["counts"])
    for key in ("vertex_id", "vertices", "labels", "colors", "faces"):
        if want[key] is None:
            assert got[key] is None, key
        else:
            assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (depth.shape, kw, key)
            assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), (depth.shape, kw, key)
    assert R.same(got, want)
    return want


def _branch_shapes():
    rc = _rc()
    px, ch = rc.block_pixels(), rc.scan_chunk()
    assert px % 2 == 0 and ch <= px                       # (ch rows of px + 1 pixels then are ch + 1 workgroups)
    return [(3, 5),                                       # less than one workgroup's pixels
            (2, px // 2), (1, px),                        # exactly one workgroup
            (1, px + 1), (3, px // 2),                    # one pixel more; one and a half
            (ch, px),                                     # as many workgroups as one step of the scan takes
            (ch, px + 1)]                                 # ... and one more


@pytest.mark.parametrize("which", range(7))
def test_sizes_that_straddle_the_launch_shapes(which):
    H, W = _branch_shapes()[which]
    depth, labels, colors, K = R.scene(H, W, seed=which, holes=0.01)
    want = _check(depth, K, labels, colors, same_label=False, max_gap=0.5)
    assert want["counts"][0] > 0 and (H == 1 or want["counts"][1] > 0)
    _check(depth, K, labels, colors)


@pytest.mark.parametrize("W", [1, 63, 64, 65, 130])
def test_widths_and_heights(W):
    for H in (1, 2, 37, 70):
        depth, labels, colors, K = R.scene(H, W, seed=H + W, holes=0.02)
        _check(depth, K, labels, colors, same_label=False, max_gap=0.5)
        _check(depth, K, labels)


def test_480_by_640():
    depth, labels, colors, K = R.scene(480, 640, seed=1, holes=0.01)
    want = _check(depth, K, labels, colors)
    assert want["counts"][0] > 290000 and want["counts"][1] > 400000


def test_options():
    depth, labels, colors, K = R.scene(37, 65, seed=8, holes=0.02)
    for kw in (dict(relative=False, max_gap=0.02), dict(same_label=False), dict(planar_only=True), dict(depth_range=(1.5, 3.0)), dict(max_gap=0.0),
               dict(planar_only=True, same_label=False, relative=False, max_gap=1.0, depth_range=(0.5, 100.0)), dict(faces=False, planar_only=True)):
        _check(depth, K, labels, colors, **kw)
    assert _check(depth, K, None, colors, planar_only=True)["counts"] == (0, 0)          # no labels: all 0
    up = np.nextafter(np.float32(2.5), np.float32(3.0))                                 # the gap rule on its boundary: 0.5 <= 0.5 is exact
    K2 = R.k_of(2.0, 2.0, 0.5, 0.5)
    for relative, gap in ((True, 0.25), (False, 0.5)):
        assert _check(np.array([[2.0, 2.0], [2.5, 2.0]], np.float32), K2, max_gap=gap, relative=relative)["counts"] == (4, 2)
        assert _check(np.array([[2.0, 2.0], [up, 2.0]], np.float32), K2, max_gap=gap, relative=relative)["counts"] == (4, 0)
        assert _check(np.array([[2.0, 2.0], [2.0, up]], np.float32), K2, max_gap=gap, relative=relative)["faces"].tolist() == [[0, 2, 1]]


PATTERNS = ["all", "none", "last pixel", "checkerboard", "last workgroup", "holes"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_validity_patterns(pattern):
    px = _rc().block_pixels()
    H, W = 37, 65
    assert H * W > 3 * px and (H * W) % px                                               # several workgroups, the last one partly filled
    depth, labels, colors, K = R.scene(H, W, seed=3, holes=0.0)
    depth = np.where(np.isfinite(depth) & (depth > 0), depth, np.float32(1.0)).astype(np.float32)
    flat = depth.reshape(-1)
    idx = np.arange(H * W)
    if pattern == "none":
        flat[:] = np.nan
    elif pattern == "last pixel":
        flat[:-1] = np.inf
    elif pattern == "checkerboard":
        flat[((idx // W + idx % W) % 2) == 1] = 0.0
    elif pattern == "last workgroup":
        flat[:(H * W) // px * px] = -1.0
    elif pattern == "holes":
        flat[np.random.RandomState(0).rand(H * W) < 0.01] = np.nan
    want = _check(depth, K, labels, colors, same_label=False, max_gap=10.0)
    nv = {"all": H * W, "none": 0, "last pixel": 1, "checkerboard": (H * W + 1) // 2, "last workgroup": (H * W) % px}.get(pattern)
    assert nv is None or want["counts"][0] == nv
    assert pattern not in ("all", "last workgroup") or want["counts"][1] > 0
    _check(depth, K, labels)


def test_ragged_batch_equals_per_image_calls():
    rc = _rc()
    H, W = 37, 65
    scenes = [R.scene(H, W, seed=s, holes=0.05 * s) for s in range(3)]
    scenes[1][0][:] = np.nan                                                             # one image all invalid
    Ks = np.stack([s[3] * np.array([[1.0 + 0.1 * i, 1, 1], [1, 1.0 - 0.05 * i, 1], [1, 1, 1]]) for i, s in enumerate(scenes)])
    d = torch.from_numpy(np.stack([s[0] for s in scenes]))[:, None].cuda()
    lab = torch.from_numpy(np.stack([s[1] for s in scenes])).cuda()
    col = torch.from_numpy(np.stack([s[2] for s in scenes])).cuda()
    m = rc.mesh(d, Ks, lab, col)
    assert m.vertices.shape == (3, H * W, 3) and m.faces.shape == (3, 2 * (H - 1) * (W - 1), 3) and m.vertices.is_cuda and m.counts.is_cuda
    batched = R.from_mesh(m)
    assert batched[1]["counts"] == (0, 0) and batched[0]["counts"] != batched[2]["counts"]
    for b in range(3):
        single = R.from_mesh(rc.mesh(d[b], torch.from_numpy(Ks[b]).cuda(), lab[b], col[b]))[0]
        assert R.same(batched[b], single) and R.same(batched[b], R.mesh_vec(scenes[b][0], Ks[b], scenes[b][1], scenes[b][2])), b


def test_point_cloud_determinism_and_untouched_inputs():
    rc = _rc()
    depth, labels, colors, K = R.scene(70, 130, seed=5, holes=0.03)
    d, l, c = _dev(depth, labels, colors)
    keep = [t.clone() for t in (d, l, c)]
    pc = rc.point_cloud(d, K, l, c)
    assert pc.faces is None and int(pc.counts[0, 1]) == 0
    assert R.same(R.from_mesh(pc)[0], R.mesh_vec(depth, K, labels, colors, faces=False))
    a, b = rc.mesh(d, K, l, c), rc.mesh(d, K, l, c)
    nv, nf = a.counts[0].tolist()
    assert torch.equal(a.counts, b.counts) and torch.equal(a.vertex_id, b.vertex_id) and torch.equal(a.faces[0, :nf], b.faces[0, :nf])
    assert torch.equal(a.vertices[0, :nv].view(torch.int32), b.vertices[0, :nv].view(torch.int32))
    assert torch.equal(a.labels[0, :nv], b.labels[0, :nv]) and torch.equal(a.colors[0, :nv], b.colors[0, :nv])
    for t, k in zip((d, l, c), keep):
        assert torch.equal(t.view(torch.uint8) if t.dtype == torch.float32 else t, k.view(torch.uint8) if k.dtype == torch.float32 else k)


def test_rows_past_the_counts_are_not_written():
    """the library writes the id map and the counts everywhere, every other buffer up to its count only"""
    from planerecnet_amd import _lib
    lib = _lib.lib
    H, W = 9, 31
    depth, labels, colors, K = R.scene(H, W, seed=2, holes=0.3)
    d, l, c = _dev(depth, labels, colors)
    k = torch.from_numpy(K.reshape(9)).cuda()
    cap, capf = H * W, 2 * (H - 1) * (W - 1)
    pat = 0x5A5A5A5A
    bufs = {"v": torch.full((cap * 3,), pat, dtype=torch.int32).cuda(), "l": torch.full((cap,), pat, dtype=torch.int32).cuda(),
            "c": torch.full((cap * 3,), 0x5A, dtype=torch.uint8).cuda(), "id": torch.full((cap,), pat, dtype=torch.int32).cuda(),
            "f": torch.full((capf * 3,), pat, dtype=torch.int32).cuda(), "n": torch.full((2,), pat, dtype=torch.int32).cuda()}
    ws = torch.empty(lib.prn_mesh_ws_bytes(1, H, W) // 4, dtype=torch.int32).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())           # noqa: E731
    st = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))
    rc = lib.prn_mesh(p(d), p(l), p(c), p(k), 1, H, W, 0.0, float("inf"), 0.05, 11, p(ws), p(bufs["v"]), p(bufs["l"]), p(bufs["c"]), p(bufs["id"]), p(bufs["f"]),
                      p(bufs["n"]), st)
    assert rc == 0, lib.prn_last_error()
    torch.cuda.synchronize()
    want = R.mesh_vec(depth, K, labels, colors)
    nv, nf = want["counts"]
    assert 0 < nv < cap and 0 < nf < capf and bufs["n"].tolist() == [nv, nf]
    assert (bufs["v"][3 * nv:] == pat).all() and (bufs["l"][nv:] == pat).all() and (bufs["c"][3 * nv:] == 0x5A).all() and (bufs["f"][3 * nf:] == pat).all()
    assert np.array_equal(bufs["v"][:3 * nv].cpu().numpy().view(np.float32).reshape(-1, 3).view(np.uint8), want["vertices"].view(np.uint8))
    assert np.array_equal(bufs["f"][:3 * nf].cpu().numpy().reshape(-1, 3), want["faces"]) and np.array_equal(bufs["c"][:3 * nv].cpu().numpy().reshape(-1, 3), want["colors"])
    assert np.array_equal(bufs["id"].cpu().numpy().reshape(H, W), want["vertex_id"])


def test_no_host_synchronisation():
    """Fails on a host implementation: that one downloads the depth."""
    rc = _rc()
    depth, labels, colors, K = R.scene(37, 65, seed=7, holes=0.02)
    d, l, c = _dev(depth, labels, colors)
    k_dev = torch.from_numpy(K).cuda()
    rc.mesh(d, K, l, c), rc.point_cloud(d, k_dev)                                        # warm: code objects loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda").item()                                          # the mode does catch a synchronisation
        full = rc.mesh(d, K, l, c)
        cloud = rc.point_cloud(d, k_dev, l)
        batch = rc.mesh(torch.stack([d, d])[:, None], K, relative=False, max_gap=0.1)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert R.same(R.from_mesh(full)[0], R.mesh_vec(depth, K, labels, colors))
    assert R.same(R.from_mesh(cloud)[0], R.mesh_vec(depth, K, labels, faces=False))
    want = R.mesh_vec(depth, K, relative=False, max_gap=0.1)
    assert all(R.same(g, want) for g in R.from_mesh(batch))


def test_library_refuses_before_any_launch():
    """with real buffers: nothing is launched, the outputs keep their fill pattern"""
    from planerecnet_amd import _lib
    lib = _lib.lib
    H, W = 4, 6
    d = torch.ones(H, W).cuda()
    lab = torch.ones(H, W, dtype=torch.int32).cuda()
    col = torch.ones(H, W, 3, dtype=torch.uint8).cuda()
    k = torch.tensor([2.0, 0, 0.5, 0, 2.0, 0.5, 0, 0, 1.0], dtype=torch.float64).cuda()
    outs = {n: torch.full((s,), -7, dtype=torch.int32).cuda() for n, s in (("v", H * W * 3), ("l", H * W), ("id", H * W), ("f", 2 * 3 * 5 * 3), ("n", 2), ("ws", 64))}
    vc = torch.full((H * W * 3,), 7, dtype=torch.uint8).cuda()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))
    inf = float("inf")

    def call(depth=d, labels=lab, colors=col, kk=k, B=1, h=H, w=W, gap=0.05, flags=11, ws=outs["ws"], v=outs["v"], vl=outs["l"], vcol=vc, vid=outs["id"],
             f=outs["f"], n=outs["n"]):
        return lib.prn_mesh(p(depth), p(labels), p(colors), p(kk), B, h, w, 0.0, inf, gap, flags, p(ws), p(v), p(vl), p(vcol), p(vid), p(f), p(n), st)

    for kw, msg in ((dict(h=4096, w=4096), b"2^24"), (dict(h=1 << 12, w=(1 << 12) + 1), b"2^24"), (dict(gap=-0.5), b"max_gap"), (dict(gap=float("nan")), b"max_gap"),
                    (dict(gap=inf), b"max_gap"), (dict(B=0), b"B <= 65535"), (dict(B=65536), b"B <= 65535"), (dict(h=0), b"positive"), (dict(w=-1), b"positive"),
                    (dict(flags=16), b"flags"), (dict(colors=None), b"together"), (dict(vcol=None), b"together"), (dict(depth=None), b"null"),
                    (dict(kk=None), b"null"), (dict(ws=None), b"null"), (dict(v=None), b"null"), (dict(vl=None), b"null"), (dict(vid=None), b"null"),
                    (dict(n=None), b"null"), (dict(f=None), b"face buffer")):
        assert call(**kw) != 0 and msg in lib.prn_last_error(), (kw, lib.prn_last_error())
    torch.cuda.synchronize()
    assert all(int((t != -7).sum()) == 0 for t in outs.values()) and int((vc != 7).sum()) == 0
    assert call() == 0 and call(f=None, flags=3) == 0                                     # the point cloud needs no face buffer
    torch.cuda.synchronize()
    assert outs["n"].tolist() == [H * W, 0] and outs["id"].tolist() == list(range(H * W)) and int((vc != 1).sum()) == 0


def test_reconstruct_results_over_planar_depth():
    """planes.planar_depth's output dicts -> the mesh of the planar depth under the owner map of the masks (restated here by painting in index order)"""
    from planerecnet_amd import planes
    rc = _rc()
    H, W = 48, 64
    rng = np.random.RandomState(11)
    results, owners, frames = [], [], []
    K = R.k_of(58.3, 57.9, 31.6, 23.7)
    for b, n in enumerate((3, 0, 2)):
        depth, _, colors, _ = R.scene(H, W, seed=20 + b, holes=0.0)
        depth = np.where(np.isfinite(depth) & (depth > 0), depth, np.float32(3.0)).astype(np.float32)
        masks = np.zeros((n, H, W), bool)
        owner = np.zeros((H, W), np.int32)
        for i in range(n):
            y0, x0 = rng.randint(0, H // 2), rng.randint(0, W // 2)
            masks[i, y0:y0 + H // 2, x0:x0 + W // 2] = True
            owner[masks[i]] = i + 1
        results.append({"pred_depth": torch.from_numpy(depth)[None, None].cuda(), "pred_masks": torch.from_numpy(masks).cuda() if n else None})
        owners.append(owner)
        frames.append(colors)
    planar = planes.planar_depth(results, K, depth_range=(0.0, 10.0))
    m = rc.reconstruct_results(planar, K, frames=frames, max_gap=0.1)
    got = R.from_mesh(m)
    flat = 0
    for b in range(3):
        pd = planar[b]["pred_plane_depth"].squeeze().cpu().numpy()
        flat += int((pd != results[b]["pred_depth"].squeeze().cpu().numpy()).sum())
        assert R.same(got[b], R.mesh_vec(pd, K, owners[b], frames[b], max_gap=0.1)), b
        d, l, c = _dev(pd, owners[b], frames[b])
        assert R.same(got[b], R.from_mesh(rc.mesh(d, K, l, c, max_gap=0.1))[0]), b
    assert flat > 0                                                                       # the planar depth is not the predicted depth
    raw = R.from_mesh(rc.reconstruct_results(results, K))                                 # the network's own dicts: pred_depth
    assert R.same(raw[1], R.mesh_vec(results[1]["pred_depth"].squeeze().cpu().numpy(), K, owners[1]))


def _ibims_inputs(folder, n=2, H=480, W=640):
    sio = pytest.importorskip("scipy.io")
    os.makedirs(folder, exist_ok=True)
    rng = np.random.RandomState(5)
    yy, xx = np.mgrid[:H, :W]
    frames = []
    for s in range(n):
        base = np.stack([128 + 100 * np.sin(xx / (40.0 + 10 * s) + c) * np.cos(yy / (55.0 + 7 * s) - c) for c in (0.0, 1.0, 2.0)], -1)
        rgb = np.clip(base + rng.randn(H, W, 3) * 10, 0, 255).astype(np.uint8)
        K = R.k_of(518.9 + s, 519.5 - s, 325.6, 253.7)
        sio.savemat(os.path.join(folder, "scene%d.mat" % s), {"data": {"rgb": rgb, "calib": K.T}})
        frames.append((rgb, K))
    return frames


def test_ibims1_pd_ply_end_to_end(tmp_path):
    """`--ibims1_pd in:out --ply`: two small .mat frames through a random-init checkpoint.  The .ply files exist; read back they equal an
    in-process reconstruct_results on the same network output, and the rules applied to the depth the exporter wrote; the vertex count is
    the number of non-NaN pixels of the exported pred_depths."""
    sio = pytest.importorskip("scipy.io")
    import simple_inference as si
    from oracle import synth
    from planerecnet_amd import planes
    from planerecnet_amd.config import cfg, set_cfg
    from planerecnet_amd.planerecnet import PlaneRecNet
    rc = _rc()
    name = "PlaneRecNet_50_config"
    set_cfg(name)
    H, W = 480, 640                                                              # (the size the exporters' own end-to-end test runs the network at)
    frames = _ibims_inputs(str(tmp_path / "in"), H=H, W=W)
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
        planar = [planes.planar_depth([r], K, depth_range=(0.0, 10.0))[0] for r, (_, K) in zip(res, frames)]
        want = [R.from_mesh(rc.reconstruct_results([pl], K, frames=[rgb], max_gap=0.1, relative=False))[0] for pl, (rgb, K) in zip(planar, frames)]
        # `--image in:out --ply --intrinsics ...` on the same network, in this process: a 96 x 128 picture, which the staging resizes five-fold
        from PIL import Image
        src, dst = str(tmp_path / "frame.png"), str(tmp_path / "shown.png")
        Image.fromarray(np.ascontiguousarray(frames[0][0][::5, ::5])).save(src)
        old_args = getattr(si, "args", None)
        try:
            a = si.parse_args(["--image", src + ":" + dst, "--ply", "--intrinsics", "103.8,103.9,65.1,50.7"])
            shown = si.inference_image(net, src, dst, depth_mode=a.depth_mode)[0]
        finally:
            si.args = old_args
        shown_depth = shown["pred_depth"][..., :H, :W].squeeze().cpu().numpy()
        shown_masks = None if shown["pred_masks"] is None else shown["pred_masks"][:, :H, :W].cpu().numpy().astype(bool)
    finally:
        cfg.solov2.replace(old)
        cfg.device = old_device
    got = rc.read_ply(str(tmp_path / "shown_mesh.ply"))
    owner = np.zeros((H, W), np.int32)
    for i in range(0 if shown_masks is None else shown_masks.shape[0]):
        owner[shown_masks[i]] = i + 1                                                    # painted in index order: the last wins
    again = R.mesh_vec(shown_depth, R.k_of(103.8 * 5, 103.9 * 5, (65.1 + 0.5) * 5 - 0.5, (50.7 + 0.5) * 5 - 0.5), owner)
    assert got["vertices"].shape[0] > 0 and got["colors"].shape == got["vertices"].shape and got["comments"] == ["PlaneRecNet frame.png"]
    for key in ("vertices", "faces", "labels"):
        assert np.array_equal(got[key].view(np.uint8), again[key].view(np.uint8)), key
    out = str(tmp_path / "out")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, os.path.join(ROOT, "simple_inference.py"), "--config", name, "--trained_model", ckpt, "--ibims1_pd", str(tmp_path / "in") + ":" + out,
           "--ply", "--ply_gap", "0.1", "--ply_absolute"]
    p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    for s, (rgb, K) in enumerate(frames):
        path = os.path.join(out, "scene%d_mesh.ply" % s)
        assert os.path.exists(path) and os.path.exists(os.path.join(out, "scene%d_results.mat" % s))
        got = rc.read_ply(path)
        exported = sio.loadmat(os.path.join(out, "scene%d_results.mat" % s))["pred_depths"]
        assert exported.dtype == np.float32 and exported.shape == (H, W)
        valid = ~np.isnan(exported)
        assert got["vertices"].shape[0] == int(valid.sum()) and got["faces"] is not None and got["colors"] is not None
        for key in ("vertices", "faces", "labels", "colors"):                            # the same network output, in this process
            assert got[key].dtype == want[s][key].dtype and np.array_equal(got[key].view(np.uint8), want[s][key].view(np.uint8)), (s, key)
        owner = np.zeros((H, W), np.int32)                                               # the rules applied to what the exporter wrote
        owner[valid] = got["labels"]
        again = R.mesh_vec(exported, K, owner, rgb, max_gap=0.1, relative=False)
        for key in ("vertices", "faces", "labels", "colors"):
            assert np.array_equal(got[key].view(np.uint8), again[key].view(np.uint8)), (s, key)
        assert np.array_equal(got["colors"], rgb[valid]) and got["labels"].max() >= 1
