"""GPU: erosion, dilation and the boundary band on the device (planerecnet_amd/morphology.py, csrc/prn_morph.hip), the boundary IoU matrix
and the boundary AP row (planerecnet_amd/metrics.py, eval.py) against the numpy restatements (tests/morphology_restate.py) and scipy.ndimage's
answers stored in tests/golden/boundary_cases.npz: image sizes round the 64-bit word and the 64-row tile of the column pass, radii inside a
word, across one, beyond the LDS form's halo and beyond the image, a ragged batch, chunking, no host synchronisation, untouched inputs.
Every comparison is exact."""
import ctypes
import io
import os
import random
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import morphology_restate as R

pytestmark = pytest.mark.gpu


def _morphology():
    from planerecnet_amd import morphology
    return morphology


def test_tile_is_what_the_sizes_below_assume():
    M = _morphology()
    assert (M.TILE_ROWS, M.TILE_WORDS, M.LDS_RADIUS) == (64, 4, 32)


T = 64
EDGE_SIZES = [(h, w) for h in (1, T - 1, T, T + 1, 2 * T + 1) for w in (1, 63, 64, 65, 129)] + [(5, 7), (37, 65)]


@pytest.mark.parametrize("h,w", EDGE_SIZES, ids=["%dx%d" % s for s in EDGE_SIZES])
def test_patterns_at_the_word_and_tile_edges(h, w):
    """every pattern of morphology_restate.patterns as one batch (an odd h * w puts most masks on an odd base address), every radius at which
    the kernels take another path, both borders, the three operations, and the areas"""
    M = _morphology()
    masks, names = R.pattern_batch(h, w)
    dev = torch.from_numpy(masks).cuda()
    for r in (0, 1, 2, 3, 31, 32, 33, 64, 65, max(h, w), max(h, w) + 7):
        for border in (0, 1):
            we, wd = R.erode_dilate(masks, r, border)
            if border == 0:
                wb = masks & ~we
            e, ea = M.erode(dev, r, border, return_area=True)
            d, da = M.dilate(dev, r, border, return_area=True)
            assert e.dtype == torch.bool and e.shape == dev.shape and ea.dtype == torch.int32 and ea.shape == (len(masks),)
            ge, gd = e.cpu().numpy(), d.cpu().numpy()
            assert np.array_equal(ge, we), ("erode", r, border, [n for n, a, b in zip(names, ge, we) if not np.array_equal(a, b)])
            assert np.array_equal(gd, wd), ("dilate", r, border, [n for n, a, b in zip(names, gd, wd) if not np.array_equal(a, b)])
            assert np.array_equal(ea.cpu().numpy(), we.reshape(len(we), -1).sum(1)) and np.array_equal(da.cpu().numpy(), wd.reshape(len(wd), -1).sum(1))
        b, ba = M.boundary(dev, r, return_area=True)
        gb = b.cpu().numpy()
        assert np.array_equal(gb, wb), ("boundary", r, [n for n, x, y in zip(names, gb, wb) if not np.array_equal(x, y)])
        assert np.array_equal(ba.cpu().numpy(), wb.reshape(len(wb), -1).sum(1))


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return R.load_fixture(os.path.join(golden_dir, "boundary_cases.npz"))


def test_fixture_cases(fixture):
    """scipy.ndimage's erosions, dilations, bands and the IoU matrices of both kinds"""
    from planerecnet_amd import metrics
    M = _morphology()
    for tag, c in fixture.items():
        for dtype in (torch.bool, torch.uint8):
            m = torch.from_numpy(c["masks"]).cuda()
            if dtype == torch.uint8:
                m = m.to(torch.uint8) * 255
            for r in c["radii"]:
                for b in (0, 1):
                    e, d = M.erode(m, r, b), M.dilate(m, r, b)
                    assert e.dtype == dtype and d.dtype == dtype and int(d.max()) <= 1 and int(e.max()) <= 1
                    assert np.array_equal(e.cpu().numpy() != 0, c["erode"][r, b]) and np.array_equal(d.cpu().numpy() != 0, c["dilate"][r, b]), (tag, r, b)
                band = M.boundary(m, r)
                assert band.dtype == dtype and int(band.max()) <= 1 and np.array_equal(band.cpu().numpy() != 0, c["band"][r]), (tag, r)
                mi, bi = metrics.boundary_iou(m[:c["split"]], m[c["split"]:], radius=r)
                assert np.array_equal(mi.cpu().numpy(), c["mask_iou"][r], equal_nan=True), (tag, r)
                assert np.array_equal(bi.cpu().numpy(), c["boundary_iou"][r], equal_nan=True), (tag, r)


@pytest.fixture(scope="module")
def frame_480():
    """20 masks of 480 x 640 and their restated bands at the metric's radius there (computed once, shared, never written)"""
    masks = R.blobs(5, 20, 480, 640, specks=12, pinholes=12)
    masks[7] = False
    masks[8] = True
    masks[9, :, :] = False
    masks[9, 0:200, 500:640] = True                                                     # clipped by the frame: a band along the frame
    bands = R.boundary(masks, 16)
    for a in (masks, bands):
        a.setflags(write=False)
    return masks, bands


def test_480x640_at_the_metric_radius(frame_480):
    M = _morphology()
    masks, bands = frame_480
    assert M.boundary_radius(480, 640) == 16
    dev = torch.tensor(masks).cuda()
    b, area = M.boundary(dev, 16, return_area=True)
    assert np.array_equal(b.cpu().numpy(), bands) and np.array_equal(area.cpu().numpy(), bands.reshape(20, -1).sum(1))
    assert bands[9, 0, 500:640].all() and bands[9, 0:200, 639].all()
    assert np.array_equal(M.erode(dev, 16, 1).cpu().numpy(), R.erode(masks, 16, 1))
    assert np.array_equal(M.dilate(dev, 16, 0).cpu().numpy(), R.dilate(masks, 16, 0))


def _ragged():
    H, W = 37, 65
    counts = (0, 3, 1, 5)
    parts = [R.blobs(40 + b, n, H, W) if n else np.zeros((0, H, W), bool) for b, n in enumerate(counts)]
    parts[3][2] = False
    parts[3][3] = True
    return parts


def test_ragged_batch_equals_per_image_calls_and_the_restatement():
    M = _morphology()
    parts = _ragged()
    dev = [torch.from_numpy(p).cuda() for p in parts]
    masks = [dev[0], dev[1], None, dev[2], dev[3]]
    for r, border in ((3, 0), (33, 1)):
        for fn, want in ((M.erode, R.erode), (M.dilate, R.dilate)):
            out, area = fn(masks, r, border, return_area=True)
            assert out[2] is None and out[0].shape == (0, 37, 65) and out[0].dtype == torch.bool and area[0].numel() == 0 and area[2].numel() == 0
            for b, p in ((1, 1), (3, 2), (4, 3)):
                o1, a1 = fn(dev[p], r, border, return_area=True)
                assert torch.equal(out[b], o1) and torch.equal(area[b], a1)
                assert np.array_equal(o1.cpu().numpy(), want(parts[p], r, border))
        band = M.boundary(masks, r)
        for b, p in ((1, 1), (3, 2), (4, 3)):
            assert torch.equal(band[b], M.boundary(dev[p], r)) and np.array_equal(band[b].cpu().numpy(), R.boundary(parts[p], r))
    nothing = M.erode([None, dev[0]], 2)
    assert nothing[0] is None and nothing[1].shape == (0, 37, 65)


def test_chunked_workspace_equals_one_call(monkeypatch):
    from planerecnet_amd import _lib
    M = _morphology()
    masks = [torch.from_numpy(p).cuda() for p in _ragged()]
    whole, warea = M.boundary(masks, 3, return_area=True)
    lib, sizes = _lib.lib, []
    real = lib.prn_morph_ws_bytes

    class Spy:
        """the library with prn_morph_ws_bytes recorded"""
        def __getattr__(self, name):
            return getattr(lib, name)

        def prn_morph_ws_bytes(self, n, H, W, radius):
            sizes.append(n)
            return real(n, H, W, radius)
    monkeypatch.setattr(_lib, "lib", Spy())
    limit = 2 * real(1, 37, 65, 3) + 8                                                 # two masks fit, three do not
    assert real(2, 37, 65, 3) <= limit < real(3, 37, 65, 3)
    chunked, carea = M.boundary(masks, 3, max_workspace_bytes=limit, return_area=True)
    assert sizes == [1, 2, 2, 2, 2, 1]                                                 # nine masks: four chunks of two (across image boundaries), one of one
    for a, b in zip(whole + warea, chunked + carea):
        assert torch.equal(a, b)
    tiny = M.boundary(masks, 3, max_workspace_bytes=1)                                 # below one mask: one mask per chunk
    assert all(torch.equal(a, b) for a, b in zip(whole, tiny))


def test_more_masks_than_one_call_takes():
    """65536 one-pixel masks: the library takes 65535 per call, the module splits"""
    M = _morphology()
    m = torch.ones(65536, 1, 1, dtype=torch.bool).cuda()
    m[77] = False
    assert torch.equal(M.erode(m, 1, 1), m) and int(M.erode(m, 1, 0).sum()) == 0
    band, area = M.boundary(m, 2, return_area=True)
    assert torch.equal(band, m) and torch.equal(area, m.view(-1).int())


def test_dtypes_untouched_inputs_and_two_runs_agree():
    M = _morphology()
    p = _ragged()[3]
    b = torch.from_numpy(p).cuda()
    weights = torch.from_numpy(np.random.RandomState(3).randint(1, 256, p.shape).astype(np.uint8)).cuda()
    u = b.to(torch.uint8) * weights                                                     # non-zero = set
    first = None
    for m in (b, u):
        before = m.clone()
        runs = [(M.erode(m, 2, 1), M.dilate(m, 33, 0), M.boundary(m, 3)) for _ in range(2)]
        assert torch.equal(m, before)
        assert all(torch.equal(x, y) for x, y in zip(*runs))
        assert all(x.dtype == m.dtype and int(x.max()) == 1 for x in runs[0])
        if first is None:
            first = runs[0]
        else:
            assert all(torch.equal(x, y != 0) for x, y in zip(first, runs[0]))
    wide = torch.zeros(b.shape[0], b.shape[1], b.shape[2] + 3, dtype=torch.bool).cuda()      # a non-contiguous view is read as what it shows
    wide[:, :, 3:] = b
    view = wide[:, :, 3:]
    assert not view.is_contiguous() and torch.equal(M.boundary(view, 3), first[2])


def test_no_host_synchronisation(frame_480):
    """Fails on a host implementation: that one downloads the masks."""
    from planerecnet_amd import metrics
    M = _morphology()
    parts = _ragged()
    masks = [torch.from_numpy(p).cuda() for p in parts]
    big = torch.tensor(frame_480[0][:4]).cuda()
    M.boundary(masks, 3), metrics.boundary_iou(big[:2], big[2:])                        # warm: code objects loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda").item()                                         # the mode does catch a synchronisation
        band = M.boundary(masks, 3)
        e = M.erode(masks[3], 40, 1, max_workspace_bytes=1)
        mi, bi = metrics.boundary_iou(big[:2], big[2:])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert np.array_equal(band[3].cpu().numpy(), R.boundary(parts[3], 3)) and np.array_equal(e.cpu().numpy(), R.erode(parts[3], 40, 1))
    assert np.array_equal(bi.cpu().numpy(), R.iou_f32(frame_480[1][:2], frame_480[1][2:4]), equal_nan=True)


def test_library_refuses_before_any_launch():
    """with real buffers: nothing is launched, nothing is written"""
    from planerecnet_amd import _lib
    lib = _lib.lib
    m = torch.ones(2, 4, 4, dtype=torch.uint8).cuda()
    ptrs = torch.tensor([m.data_ptr()], dtype=torch.int64).cuda()
    first = torch.tensor([0, 2], dtype=torch.int32).cuda()
    out = torch.full((8,), -7, dtype=torch.int32).cuda()                                # 32 bytes
    area = torch.full((2,), -7, dtype=torch.int32).cuda()
    ws = torch.empty(lib.prn_morph_ws_bytes(2, 4, 4, 1) // 4 + 2, dtype=torch.int32).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))
    for args, msg in (((1, 2, 1 << 16, 1 << 15, 0, 1, 0), b"2^31"), ((1, 65536, 4, 4, 0, 1, 0), b"65535"), ((1, 2, 4, 4, 3, 1, 0), b"op must be"),
                      ((1, 0, 4, 4, 0, 1, 0), b"Ntot"), ((1, 2, 4, 4, 0, -1, 0), b"radius"), ((1, 2, 4, 4, 0, 1, 2), b"border")):
        assert lib.prn_morph(p(ptrs), p(first), *args, p(out), p(area), p(ws), st) != 0 and msg in lib.prn_last_error()
    assert lib.prn_morph(p(ptrs), p(first), 1, 2, 4, 4, 0, 1, 0, p(out), p(area), ctypes.c_void_p(ws.data_ptr() + 4), st) != 0
    assert b"aligned" in lib.prn_last_error()
    torch.cuda.synchronize()
    assert int((out != -7).sum()) == 0 and int((area != -7).sum()) == 0
    assert lib.prn_morph(p(ptrs), p(first), 1, 2, 4, 4, 0, 1, 1, p(out), p(area), p(ws), st) == 0
    assert torch.equal(out.view(torch.uint8), torch.ones(32, dtype=torch.uint8).cuda()) and area.tolist() == [16, 16]


# ---- metrics.boundary_iou ----------------------------------------------------------------------------------------------------------

IOU_SIZES = [(1, 1), (63, 63), (64, 64), (65, 65), (37, 129), (129, 65)]


@pytest.mark.parametrize("h,w", IOU_SIZES, ids=["%dx%d" % s for s in IOU_SIZES])
def test_boundary_iou_at_the_word_edges(h, w):
    from planerecnet_amd import metrics
    M = _morphology()
    masks, names = R.pattern_batch(h, w)
    pool = np.concatenate([masks, R.blobs(9, 12, h, w)])
    rng = np.random.RandomState(h * 131 + w)
    r = M.boundary_radius(h, w) if min(h, w) > 1 else 1
    for A, B in ((1, 1), (3, 17), (17, 3), (17, 17)):
        a, b = pool[rng.choice(len(pool), A)], pool[rng.choice(len(pool), B)]
        a[0], b[-1] = False, False                                                       # one 0/0 (NaN); an empty mask against a set one is 0
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        for radius in (r, 2, 40):
            mi, bi = metrics.boundary_iou(da, db, radius=radius)
            assert mi.shape == (A, B) and bi.shape == (A, B) and mi.dtype == torch.float32 and bi.dtype == torch.float32
            plain = metrics.pairwise_iou(da, db)[0]
            assert np.array_equal(mi.cpu().numpy().view(np.uint32), plain.cpu().numpy().view(np.uint32))          # bit-identical, NaN included
            wm, wb = R.boundary_ious(a, b, radius)
            assert np.array_equal(mi.cpu().numpy(), wm, equal_nan=True) and np.array_equal(bi.cpu().numpy(), wb, equal_nan=True), (A, B, radius)
            assert np.isnan(bi[0, -1].item()) and np.isnan(mi[0, -1].item())
        d1, d2 = metrics.boundary_iou(da, db)                                            # radius=None: the mask size's own
        want = metrics.boundary_iou(da, db, radius=M.boundary_radius(h, w))
        assert torch.equal(d1.view(torch.int32), want[0].view(torch.int32)) and torch.equal(d2.view(torch.int32), want[1].view(torch.int32))


def test_boundary_iou_480x640(frame_480):
    from planerecnet_amd import metrics
    masks, bands = frame_480
    a, b = torch.tensor(masks).cuda(), torch.tensor(masks[5:20]).cuda()
    mi, bi = metrics.boundary_iou(a, b)
    assert mi.shape == (20, 15)
    assert np.array_equal(mi.cpu().numpy().view(np.uint32), metrics.pairwise_iou(a, b)[0].cpu().numpy().view(np.uint32))
    assert np.array_equal(bi.cpu().numpy(), R.iou_f32(bands, bands[5:20]), equal_nan=True)
    assert np.isnan(bi[7, 2].item()) and float(bi[6, 1]) == 1.0                       # mask 7 is empty; mask 6 against itself
    u = a.to(torch.uint8) * 200
    m2, b2 = metrics.boundary_iou(u, b.float())                                         # other dtypes: non-zero = set
    assert torch.equal(m2.view(torch.int32), mi.view(torch.int32)) and torch.equal(b2.view(torch.int32), bi.view(torch.int32))


def test_boundary_iou_empty_sets_and_refusals():
    from planerecnet_amd import metrics
    z, m = torch.zeros(0, 9, 9, dtype=torch.bool).cuda(), torch.ones(3, 9, 9, dtype=torch.bool).cuda()
    for a, b in ((z, m), (m, z), (z, z)):
        mi, bi = metrics.boundary_iou(a, b)
        assert mi.shape == (a.shape[0], b.shape[0]) == bi.shape and mi.is_cuda and mi.dtype == torch.float32
    with pytest.raises(RuntimeError, match="different size"):
        metrics.boundary_iou(m, torch.ones(3, 9, 8, dtype=torch.bool).cuda())
    with pytest.raises(RuntimeError, match="device"):
        metrics.boundary_iou(m.cpu(), m.cpu())
    with pytest.raises(ValueError, match="radius"):
        metrics.boundary_iou(m, m, radius=-1)


# ---- boundary AP -------------------------------------------------------------------------------------------------------------------

def _pushed(ap):
    return {k: [(o.scores, o.hits, o.num_gt_positives) for o in v] for k, v in ap.items()}


def test_compute_segmentation_metrics_with_the_boundary_radius():
    from planerecnet_amd import metrics
    gt, det, scores = R.shifted_rectangles()
    gt_d, det_d = torch.from_numpy(gt).cuda(), torch.from_numpy(det).cuda()
    gt_boxes, det_boxes = metrics.mask_boxes(gt_d), metrics.mask_boxes(det_d).cpu()
    args = (gt_d, gt_boxes, torch.zeros(1), det_d, det_boxes, torch.zeros(3), torch.from_numpy(scores))
    plain = metrics.new_ap_data()
    metrics.compute_segmentation_metrics(plain, *args)
    ap = metrics.new_ap_data(boundary=True)
    metrics.compute_segmentation_metrics(ap, *args, boundary_radius=3)
    got, want = _pushed(ap), _pushed(plain)
    assert got["box"] == want["box"] and got["mask"] == want["mask"]
    mi, bi = R.boundary_ious(det, gt, 3)
    for t, thr in enumerate(metrics.iou_thresholds):
        o = ap["boundary"][t]
        assert list(zip(o.scores, o.hits)) == R.ap_pushes(R.boundary_ap_iou(mi, bi), scores, thr) and o.num_gt_positives == 1
    hits = [[h for s, h in zip(o.scores, o.hits) if s == sc and h] for o in ap["boundary"] for sc in (0.7, 0.8, 0.9)]
    assert sum(len(h) for h in hits) == 10 + 1 + 0                                      # up to .95 / .50 / none
    table = metrics.calc_map(ap, quiet=True)
    assert table["boundary"]["all"] < table["mask"]["all"]


class _StubNet(torch.nn.Module):
    """returns a prepared eval-mode result for the frame whose number the image carries"""

    def __init__(self, results):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.results = results

    def forward(self, x):
        return [self.results[int(x[0, 0, 0, 0].item())]]


class _StubDataset:
    def __init__(self, frames):
        self.frames = frames

    def __len__(self):
        return len(self.frames)

    def pull_item(self, i):
        return self.frames[i]


def _stub_eval():
    from planerecnet_amd import metrics
    H, W = 96, 128
    gt, det, scores = R.shifted_rectangles()
    frames, results = [], []
    for i in range(3):
        g = np.roll(gt, 5 * i, axis=2)
        d = np.roll(det, 5 * i, axis=2)[:3 - i] if i < 2 else np.roll(det, 5 * i, axis=2)[1:]
        sc = scores[:len(d)]
        gm = torch.from_numpy(g)
        image = torch.full((3, H, W), float(i))
        depth = torch.full((1, H, W), 2.0 + i)
        frames.append((image, {"masks": gm, "boxes": metrics.mask_boxes(gm.cuda()).cpu(), "classes": torch.zeros(1)}, depth))
        dm = torch.from_numpy(d).cuda()
        results.append({"pred_masks": dm, "pred_boxes": metrics.mask_boxes(dm).cpu(), "pred_classes": torch.zeros(len(d)).cuda(),
                        "pred_scores": torch.from_numpy(sc).cuda(), "pred_depth": (depth * 1.1).cuda()})
    return _StubNet(results).cuda(), _StubDataset(frames), frames, results


def test_evaluate_end_to_end():
    import eval as ev
    from planerecnet_amd import metrics
    net, dataset, frames, results = _stub_eval()
    ev.parse_args(["--no_bar"])
    with torch.no_grad():
        random.seed(0)
        buf = io.StringIO()
        with redirect_stdout(buf):
            table, depth = ev.evaluate(net, dataset, eval_nums=3, boundary_ratio=0.02)
        assert list(table) == ["box", "mask", "boundary"] and list(table["boundary"]) == list(table["mask"])
        assert table["boundary"]["all"] <= table["mask"]["all"] and table["boundary"]["all"] < 100.0
        assert "bndry |" in buf.getvalue() and abs(depth["abs_rel"] - 0.1) < 1e-5
        random.seed(0)
        plain_buf = io.StringIO()
        with redirect_stdout(plain_buf):
            plain, pdepth = ev.evaluate(net, dataset, eval_nums=3)
    assert list(plain) == ["box", "mask"] and plain["box"] == table["box"] and plain["mask"] == table["mask"] and pdepth == depth
    # the parent's code path, frame by frame in the same order: the same table and the same text
    random.seed(0)
    order = list(range(3))
    random.shuffle(order)
    ap = metrics.new_ap_data()
    for i in order:
        g, r = frames[i][1], results[i]
        metrics.compute_segmentation_metrics(ap, g["masks"].cuda(), g["boxes"].cuda(), g["classes"], r["pred_masks"], r["pred_boxes"], r["pred_classes"],
                                             r["pred_scores"])
    want_buf = io.StringIO()
    with redirect_stdout(want_buf):
        want = metrics.calc_map(ap)
    assert want == plain and want_buf.getvalue() in plain_buf.getvalue() and "bndry" not in plain_buf.getvalue()
    assert [ln for ln in buf.getvalue().splitlines() if "bndry" not in ln] == plain_buf.getvalue().splitlines()
