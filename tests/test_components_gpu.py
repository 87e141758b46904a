"""GPU: connected components and mask cleaning on the device (planerecnet_amd/components.py, csrc/prn_ccl.hip) against the numpy
restatements (tests/components_restate.py) and scipy.ndimage's answers stored in tests/golden/components_cases.npz: image sizes round the
32 x 64 tile of the LDS union-find, the shapes at which each launch can go wrong, a ragged batch, chunking, no host synchronisation,
untouched inputs, clean_results and planar_depth(clean=...).  Every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

import components_restate as R
from planes_restate import k_of, plane_depth_map

pytestmark = pytest.mark.gpu

NAMES = ("count", "kept", "largest", "area")


def _components():
    from planerecnet_amd import components
    return components


def _info(info):
    return np.stack([info[k].cpu().numpy() for k in NAMES])


def _winfo(info):
    return np.stack([info[k] for k in NAMES])


def test_tile_is_what_the_sizes_below_assume():
    assert _components().TILE == (32, 64)


TH, TW = 32, 64
EDGE_SIZES = [(h, w) for h in (1, TH - 1, TH, TH + 1, 2 * TH + 1) for w in (1, TW - 1, TW, TW + 1, 2 * TW + 1)] + [(5, 7), (37, 65)]
# per size: the selections whose restatement is cheap enough to run everywhere; (37, 65) and the fixture run all of CLEAN_VARIANTS
VARIANTS = (("largest", 0, True), ("all", 5, False), ("all", 5, True))


@pytest.mark.parametrize("h,w", EDGE_SIZES, ids=["%dx%d" % s for s in EDGE_SIZES])
def test_patterns_at_the_tile_edges(h, w):
    """every pattern of components_restate.patterns as one batch, both connectivities: labels, counts, cleaned masks and statistics.
    Odd H * W puts most masks of the batch on an odd base address."""
    C = _components()
    P = R.patterns(h, w)
    masks = np.stack([P[k] for k in sorted(P)])
    dev = torch.from_numpy(masks).cuda()
    for conn in (4, 8):
        want, cnt = R.label_flood_batch(masks, conn)
        labels, count = C.label(dev, conn)
        assert labels.dtype == torch.int32 and labels.shape == dev.shape and count.dtype == torch.int32
        assert np.array_equal(count.cpu().numpy(), cnt), (conn, sorted(P), count.cpu().numpy(), cnt)
        assert np.array_equal(labels.cpu().numpy(), want), conn
        for keep, min_area, fill in (R.CLEAN_VARIANTS if (h, w) == (37, 65) else VARIANTS):
            wmask, winfo = R.clean_batch(masks, conn, keep, min_area, fill, label=R.label_flood)
            out, info = C.clean(dev, conn, keep=keep, min_area=min_area, fill_holes=fill)
            assert out.dtype == torch.bool and out.shape == dev.shape
            assert np.array_equal(_info(info), _winfo(winfo)), (conn, keep, min_area, fill)
            assert np.array_equal(out.cpu().numpy(), wmask), (conn, keep, min_area, fill)


def test_fixture_cases(golden_dir):
    """scipy.ndimage's labels and cleaned masks (label, bincount, binary_fill_holes with the dual structure)"""
    C = _components()
    for tag, c in R.load_fixture(os.path.join(golden_dir, "components_cases.npz")).items():
        for dtype in (torch.bool, torch.uint8):
            m = torch.from_numpy(c["masks"]).cuda()
            if dtype == torch.uint8:
                m = m.to(torch.uint8) * 255
            for conn in (4, 8):
                labels, count = C.label(m, conn)
                assert np.array_equal(labels.cpu().numpy(), c["labels"][conn]) and np.array_equal(count.cpu().numpy(), c["count"][conn]), (tag, conn)
                for v, (keep, min_area, fill) in enumerate(R.CLEAN_VARIANTS):
                    out, info = C.clean(m, conn, keep=keep, min_area=min_area, fill_holes=fill)
                    assert out.dtype == dtype and int(out.max()) <= 1
                    assert np.array_equal(out.cpu().numpy() != 0, c["clean"][conn, v]), (tag, conn, v)
                    assert np.array_equal(_info(info), c["info"][conn, v]), (tag, conn, v)


def test_ties_and_min_area_at_the_edges():
    """two and three components of equal maximal area: the lowest label wins; min_area exactly at, one below and one above an area"""
    C = _components()
    for h, w in ((33, 65), (37, 65)):
        P = R.patterns(h, w, densities=())
        for conn in (4, 8):
            for name in ("tie2", "tie3"):
                lab, _ = R.label_flood(P[name], conn)
                out, info = C.clean(torch.from_numpy(P[name][None]).cuda(), conn)
                assert np.array_equal(out[0].cpu().numpy(), lab == 2)                  # (label 1 is the single pixel before them)
                assert _info(info)[:, 0].tolist() == [3 if name == "tie2" else 4, 1, 6, 6]
            m = torch.from_numpy(P["areas_6_4_1"][None]).cuda()
            for min_area, kept in ((5, 1), (6, 1), (7, 0), (4, 2), (1, 3), (0, 3)):
                out, info = C.clean(m, conn, keep="all", min_area=min_area)
                want, winfo = R.clean(P["areas_6_4_1"], conn, "all", min_area, False, label=R.label_flood)
                assert np.array_equal(out[0].cpu().numpy(), want) and _info(info)[:, 0].tolist() == [winfo[k] for k in NAMES]
                assert int(info["kept"][0]) == kept
                out, info = C.clean(m, conn, keep="largest", min_area=min_area)
                assert _info(info)[:, 0].tolist() == [3, int(min_area <= 6), 6, 6 * int(min_area <= 6)]
                assert int(out.sum()) == 6 * int(min_area <= 6)


def test_120x160():
    C = _components()
    P = R.patterns(120, 160)
    masks = np.stack([P[k] for k in sorted(P)])
    dev = torch.from_numpy(masks).cuda()
    for conn in (4, 8):
        want, cnt = R.label_flood_batch(masks, conn)
        labels, count = C.label(dev, conn)
        assert np.array_equal(count.cpu().numpy(), cnt) and np.array_equal(labels.cpu().numpy(), want)
    wmask, winfo = R.clean_batch(masks, 8, "largest", 0, True, label=R.label_flood)
    out, info = C.clean(dev, 8, fill_holes=True)
    assert np.array_equal(out.cpu().numpy(), wmask) and np.array_equal(_info(info), _winfo(winfo))


def test_480x640():
    """the inference size: 150 tiles per mask, chains of > 10^5 pixels across every seam (serpentine, spiral), a ragged 4-connected cluster
    near the percolation threshold, and a blob with specks and pin-holes.  Reference: the flood fill."""
    C = _components()
    H, W = 480, 640
    P = R.patterns(H, W, densities=(0.59,))
    blob = R.blobs(7, 1, H, W)[0]
    masks = np.stack([blob, P["random_0.59"], P["serpentine_v"], P["spiral"]])
    dev = torch.from_numpy(masks).cuda()
    labels, count = C.label(dev, 4)
    for n in range(4):
        want, k = R.label_flood(masks[n], 4)
        assert int(count[n]) == k and np.array_equal(labels[n].cpu().numpy(), want), n
    assert int(count[2]) == 1 and int(count[3]) == 1
    out, info = C.clean(dev, 8, keep="largest", fill_holes=True)
    got = out.cpu().numpy()
    for n in (0, 1):
        want, winfo = R.clean(masks[n], 8, "largest", 0, True, label=R.label_flood)
        assert np.array_equal(got[n], want) and _info(info)[:, n].tolist() == [winfo[k] for k in NAMES], n
    assert np.array_equal(got[2], masks[2]) and np.array_equal(got[3], masks[3])     # one component without a hole: unchanged
    assert _info(info)[:, 2].tolist() == [1, 1, int(masks[2].sum()), int(masks[2].sum())]


def _ragged():
    rng = np.random.RandomState(11)
    H, W = 37, 65
    counts = (3, 0, 1, 17)
    parts = [R.blobs(40 + b, n, H, W, specks=6, pinholes=6) if n else np.zeros((0, H, W), bool) for b, n in enumerate(counts)]
    parts[3][5] = rng.rand(H, W) < 0.59
    parts[3][6] = False
    return parts


def test_ragged_batch_equals_per_image_calls_and_the_restatement():
    C = _components()
    parts = _ragged()
    dev = [torch.from_numpy(p).cuda() for p in parts]
    masks = [dev[0], None, dev[1], dev[2], dev[3]]
    labels, count = C.label(masks, 8)
    out, info = C.clean(masks, 8, keep="all", min_area=3, fill_holes=True)
    assert labels[1] is None and out[1] is None and count[1].numel() == 0 and info["kept"][1].numel() == 0
    assert labels[2].shape == (0, 37, 65) and out[2].shape == (0, 37, 65) and out[2].dtype == torch.bool and count[2].numel() == 0
    for b, p in ((0, 0), (3, 2), (4, 3)):
        l1, c1 = C.label(dev[p], 8)
        o1, i1 = C.clean(dev[p], 8, keep="all", min_area=3, fill_holes=True)
        assert torch.equal(labels[b], l1) and torch.equal(count[b], c1) and torch.equal(out[b], o1)
        assert all(torch.equal(info[k][b], i1[k]) for k in NAMES)
        want, cnt = R.label_flood_batch(parts[p], 8)
        wmask, winfo = R.clean_batch(parts[p], 8, "all", 3, True, label=R.label_flood)
        assert np.array_equal(l1.cpu().numpy(), want) and np.array_equal(c1.cpu().numpy(), cnt)
        assert np.array_equal(o1.cpu().numpy(), wmask) and np.array_equal(_info(i1), _winfo(winfo))
    nothing, ninfo = C.clean([None, dev[1]])
    assert nothing[0] is None and nothing[1].shape == (0, 37, 65) and ninfo["count"][1].numel() == 0


def test_chunked_workspace_equals_one_call(monkeypatch):
    from planerecnet_amd import _lib
    C = _components()
    parts = _ragged()
    masks = [torch.from_numpy(p).cuda() for p in parts]
    whole, winfo = C.clean(masks, 4, keep="all", min_area=2, fill_holes=True)
    lib, sizes = _lib.lib, []
    real = lib.prn_ccl_ws_bytes

    class Spy:
        """the library with prn_ccl_ws_bytes recorded"""
        def __getattr__(self, name):
            return getattr(lib, name)

        def prn_ccl_ws_bytes(self, n, H, W):
            sizes.append(n)
            return real(n, H, W)
    monkeypatch.setattr(_lib, "lib", Spy())
    limit = 2 * real(1, 37, 65) + 8                                                    # two masks fit, three do not
    assert real(2, 37, 65) <= limit < real(3, 37, 65)
    chunked, cinfo = C.clean(masks, 4, keep="all", min_area=2, fill_holes=True, max_workspace_bytes=limit)
    assert [n for n in sizes if n != 1].count(2) == 10 and max(sizes) == 2             # 21 masks: ten chunks of two (across image boundaries) and one of one
    for a, b in zip(whole, chunked):
        assert torch.equal(a, b)
    for k in NAMES:
        for a, b in zip(winfo[k], cinfo[k]):
            assert torch.equal(a, b)
    tiny, tinfo = C.clean(masks, 4, keep="all", min_area=2, fill_holes=True, max_workspace_bytes=1)      # below one mask: one mask per chunk
    assert all(torch.equal(a, b) for a, b in zip(whole, tiny))


def test_more_masks_than_one_call_takes():
    """65536 one-pixel masks: the library takes 65535 per call, the module splits"""
    C = _components()
    m = torch.ones(65536, 1, 1, dtype=torch.bool).cuda()
    m[77] = False
    labels, count = C.label(m, 4)
    assert torch.equal(labels.view(-1), m.view(-1).int()) and torch.equal(count, m.view(-1).int())
    out, info = C.clean(m, fill_holes=True)
    assert torch.equal(out, m) and torch.equal(info["area"], m.view(-1).int())


def test_dtypes_untouched_inputs_and_two_runs_agree():
    C = _components()
    parts = _ragged()
    b = torch.from_numpy(parts[3]).cuda()
    weights = torch.from_numpy(np.random.RandomState(3).randint(1, 256, parts[3].shape).astype(np.uint8)).cuda()
    u = b.to(torch.uint8) * weights                                                     # non-zero = set
    first = None
    for m in (b, u):
        before = m.clone()
        runs = [(C.label(m, 8), C.clean(m, 8, fill_holes=True)) for _ in range(2)]
        assert torch.equal(m, before)
        (l0, c0), (o0, i0) = runs[0]
        (l1, c1), (o1, i1) = runs[1]
        assert torch.equal(l0, l1) and torch.equal(c0, c1) and torch.equal(o0, o1) and all(torch.equal(i0[k], i1[k]) for k in NAMES)
        assert o0.dtype == m.dtype and int(o0.max()) == 1
        if first is None:
            first = (l0, c0, o0, i0)
        else:
            assert torch.equal(first[0], l0) and torch.equal(first[1], c0) and torch.equal(first[2], o0 != 0)
            assert all(torch.equal(first[3][k], i0[k]) for k in NAMES)
    wide = torch.zeros(b.shape[0], b.shape[1], b.shape[2] + 3, dtype=torch.bool).cuda()      # a non-contiguous view is read as what it shows
    wide[:, :, 3:] = b
    view = wide[:, :, 3:]
    assert not view.is_contiguous()
    assert torch.equal(C.label(view, 8)[0], first[0]) and torch.equal(C.clean(view, 8, fill_holes=True)[0], first[2])


def test_no_host_synchronisation():
    """Fails on a host implementation: that one downloads the masks."""
    C = _components()
    parts = _ragged()
    masks = [torch.from_numpy(p).cuda() for p in parts]
    want, _ = R.clean_batch(parts[3], 8, "largest", 0, True, label=R.label_flood)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda").item()                                         # the mode does catch a synchronisation
        labels, count = C.label(masks, 8)
        out, info = C.clean(masks, 8, fill_holes=True)
        one, _ = C.clean(masks[3], 8, fill_holes=True, max_workspace_bytes=1)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert np.array_equal(out[3].cpu().numpy(), want) and torch.equal(one, out[3])
    assert np.array_equal(count[3].cpu().numpy(), R.label_flood_batch(parts[3], 8)[1])


def test_refusals():
    from planerecnet_amd import _lib
    C = _components()
    lib = _lib.lib
    m = torch.ones(2, 4, 4, dtype=torch.bool).cuda()
    with pytest.raises(RuntimeError, match=r"masks\[1\]"):
        C.clean([m, m.cpu()])
    with pytest.raises(RuntimeError, match="float32"):
        C.label(m.float())
    with pytest.raises(RuntimeError, match="connectivity"):
        C.clean(m, connectivity=6)
    # the library itself, with real buffers: nothing is launched, nothing is written
    ptrs = torch.tensor([m.data_ptr()], dtype=torch.int64).cuda()
    first = torch.tensor([0, 2], dtype=torch.int32).cuda()
    labels = torch.full((2, 4, 4), -7, dtype=torch.int32).cuda()
    count = torch.full((2,), -7, dtype=torch.int32).cuda()
    ws = torch.empty(lib.prn_ccl_ws_bytes(2, 4, 4) // 4 + 2, dtype=torch.int32).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))
    for args, msg in (((1, 2, 1 << 16, 1 << 15, 8), b"2^31"), ((1, 65536, 4, 4, 8), b"65535"), ((1, 2, 4, 4, 5), b"connectivity"), ((1, 0, 4, 4, 8), b"Ntot")):
        assert lib.prn_ccl_label(p(ptrs), p(first), *args, p(labels), p(count), p(ws), st) != 0 and msg in lib.prn_last_error()
    assert lib.prn_ccl_label(p(ptrs), p(first), 1, 2, 4, 4, 8, p(labels), p(count), ctypes.c_void_p(ws.data_ptr() + 4), st) != 0
    assert b"aligned" in lib.prn_last_error()
    torch.cuda.synchronize()
    assert int((labels != -7).sum()) == 0 and int((count != -7).sum()) == 0
    assert lib.prn_ccl_label(p(ptrs), p(first), 1, 2, 4, 4, 8, p(labels), p(count), p(ws), st) == 0
    assert torch.equal(labels, torch.ones_like(labels)) and count.tolist() == [1, 1]


def _results():
    rng = np.random.RandomState(21)
    H, W = 66, 130
    out = []
    for b, n in enumerate((4, 0, 2)):
        if n == 0:
            out.append({"pred_masks": None, "pred_boxes": None, "pred_classes": None, "pred_scores": None, "pred_depth": torch.rand(1, 1, H, W).cuda()})
            continue
        m = R.blobs(60 + b, n, H, W, specks=5, pinholes=5)
        if b == 2:
            m[1] = False
            m[1, 3, 5] = True                                                           # one pixel: min_area empties it
        out.append({"pred_masks": torch.from_numpy(m).cuda(), "pred_boxes": torch.zeros(n, 4), "pred_classes": torch.arange(n).cuda(),
                    "pred_scores": torch.from_numpy(rng.rand(n)).cuda(), "pred_depth": torch.rand(1, 1, H, W).cuda()})
    return out


def test_clean_results():
    from planerecnet_amd.metrics import mask_boxes
    C = _components()
    results = _results()
    keep_masks = [None if r["pred_masks"] is None else r["pred_masks"].clone() for r in results]
    new = C.clean_results(results, keep="largest", min_area=2, fill_holes=True)
    assert len(new) == 3 and all(a is not b for a, b in zip(new, results))
    assert new[1]["pred_masks"] is None and new[1]["pred_boxes"] is None and new[1]["pred_depth"] is results[1]["pred_depth"]
    for b in (0, 2):
        want, winfo = R.clean_batch(keep_masks[b].cpu().numpy(), 8, "largest", 2, True, label=R.label_flood)
        assert np.array_equal(new[b]["pred_masks"].cpu().numpy(), want)
        assert new[b]["pred_masks"].dtype == torch.bool and new[b]["pred_masks"].is_cuda
        assert not new[b]["pred_boxes"].is_cuda
        assert torch.equal(new[b]["pred_boxes"], mask_boxes(torch.from_numpy(want).cuda()).cpu())
        for key in ("pred_classes", "pred_scores", "pred_depth"):
            assert new[b][key] is results[b][key]
        assert torch.equal(results[b]["pred_masks"], keep_masks[b]) and torch.equal(results[b]["pred_boxes"], torch.zeros_like(results[b]["pred_boxes"]))
    assert int(new[2]["pred_masks"][1].sum()) == 0                                      # emptied, not dropped
    assert new[2]["pred_masks"].shape[0] == 2 and new[2]["pred_boxes"].shape == (2, 4)
    # one synchronisation: the box download
    torch.cuda.synchronize()
    none = C.clean_results([results[1]])
    assert none[0]["pred_masks"] is None and none[0] is not results[1]


def test_planar_depth_with_cleaned_masks_on_exact_planes():
    """A box on plane A plus a 3 x 3 speck on plane B at another depth: with clean=dict(keep="largest") the fitted plane meets the bounds of
    test_planes_gpu.py::test_exact_planes_are_recovered (1e-5 rad, 1e-5 relative in d); without it the speck tilts the plane beyond them."""
    from planerecnet_amd import planes
    H, W = 96, 128
    K = k_of(110.0, 100.0, 63.5, 47.5)
    nA, dA = np.asarray([0.3, -0.5, 1.0]) / np.linalg.norm([0.3, -0.5, 1.0]), 2.0
    nB, dB = np.asarray([0.0, 0.0, 1.0]), 4.0
    depth = plane_depth_map(nA, dA, K, H, W)
    far = plane_depth_map(nB, dB, K, H, W)
    depth[5:8, 110:113] = far[5:8, 110:113]
    assert (depth > 0).all()
    mask = np.zeros((1, H, W), bool)
    mask[0, 20:70, 20:90] = True
    mask[0, 5:8, 110:113] = True
    result = {"pred_masks": torch.from_numpy(mask).cuda(), "pred_boxes": torch.zeros(1, 4), "pred_classes": torch.zeros(1).cuda(),
              "pred_scores": torch.ones(1).cuda(), "pred_depth": torch.from_numpy(depth.astype(np.float32))[None, None].cuda()}

    def angle(p):
        return float(np.arccos(min(1.0, float(p[:3] @ nA))))

    cleaned = planes.planar_depth([result], K, clean=dict(keep="largest"))[0]
    p = cleaned["pred_planes"][0].cpu().numpy()
    assert bool(cleaned["pred_plane_valid"][0])
    print("cleaned: angle %.3e rad, d error %.3e relative" % (angle(p), abs(float(p[3]) - dA) / dA))
    assert angle(p) <= 1e-5 and abs(float(p[3]) - dA) <= 1e-5 * dA
    want, _ = R.clean(mask[0], 8, "largest", 0, False, label=R.label_flood)
    assert np.array_equal(cleaned["pred_plane_masks"][0].cpu().numpy(), want) and int(want.sum()) == 50 * 70
    assert torch.equal(cleaned["pred_masks"], result["pred_masks"])                     # the detection's own mask stays
    raw = planes.planar_depth([result], K)[0]
    assert "pred_plane_masks" not in raw
    q = raw["pred_planes"][0].cpu().numpy()
    print("as predicted: angle %.3e rad" % angle(q))
    assert angle(q) > 1e-5                                                              # the test sees the speck
    # the composition paints the plane over the cleaned mask only
    pd = cleaned["pred_plane_depth"][0, 0].cpu().numpy()
    assert np.array_equal(pd[5:8, 110:113], depth.astype(np.float32)[5:8, 110:113])
