"""CPU: plane-level evaluation (planerecnet_amd/plane_eval.py) without a GPU -- the scores and curves from hand-made tables, the table
formulation against the dense broadcast restatement (tests/plane_eval_restate.py), the numpy path of label_map / overlap against the per-pixel
restatement, and eval.py's flag."""
import math

import numpy as np
import pytest
import torch

import plane_eval_restate as R


def _pe():
    from planerecnet_amd import plane_eval
    return plane_eval


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all(np.abs(a - b)[~np.isnan(a)] <= tol * np.maximum(1.0, np.abs(b)[~np.isnan(a)])))


def test_constants_match_the_library():
    from planerecnet_amd import _lib
    P = _pe()
    assert P.LDS_BINS == _lib.lib.prn_label_overlap_lds_bins() == 4096 and P.MAX_LABEL == 1023 and P.DEPTH_SCALE == 2 ** 20
    assert np.array_equal(P.THRESHOLDS, 0.05 * np.arange(21))


# ---- scores from tables, hand values -------------------------------------------------------------------------------------------------

def test_identical_maps_score_1_0_1():
    P = _pe()
    T = np.diag([40, 10, 25, 7]).astype(np.int64)                   # label 0 meets label 0, and three planes meet themselves
    assert P.segmentation_scores(T) == (1.0, 0.0, 1.0)
    S = T * (P.DEPTH_SCALE // 10)                                    # every pair 0.1 m off (rounded down: D <= 0.1)
    plane, pixel = P.recall_curves(T, S)
    assert plane.shape == (21,) and pixel.shape == (21,)
    assert np.array_equal(plane, (P.THRESHOLDS >= 0.1 - 1e-9).astype(float)) and np.array_equal(pixel, plane)


@pytest.mark.parametrize("n", [2, 10, 4096])
def test_two_halves_against_one_segment(n):
    P = _pe()
    T = np.array([[0, 0], [0, n // 2], [0, n // 2]], np.int64)
    ri, voi, sc = P.segmentation_scores(T)
    assert abs(ri - (n - 2) / (2.0 * (n - 1))) <= 1e-15 and voi == 1.0 and sc == 0.5
    # a prediction of nothing: column 0 is that segment -- the same scores, and nothing is recalled
    T0 = np.array([[5], [n // 2], [n // 2]], np.int64)
    assert P.segmentation_scores(T0) == (ri, voi, sc)
    plane, pixel = P.recall_curves(T0, np.zeros_like(T0))
    assert np.array_equal(plane, np.zeros(21)) and np.array_equal(pixel, np.zeros(21))
    Tw = np.array([[5, 0], [n // 2, 0], [n // 2, 0]], np.int64)       # a detection that claims no pixel changes nothing
    assert P.segmentation_scores(Tw) == (ri, voi, sc)


def test_row_0_is_dropped_and_few_pixels_give_nan():
    P = _pe()
    T = np.array([[1000, 300, 7], [0, 30, 0], [2, 0, 50]], np.int64)
    T2 = T.copy()
    T2[0] = (1, 2, 3)
    assert P.segmentation_scores(T) == P.segmentation_scores(T2)
    for t in (np.zeros((3, 3), np.int64), np.array([[9, 9], [0, 1]], np.int64), np.zeros((1, 4), np.int64)):
        assert all(math.isnan(v) for v in P.segmentation_scores(t))
    plane, pixel = P.recall_curves(np.array([[7, 3]], np.int64), np.zeros((1, 2), np.int64))      # no ground-truth plane
    assert np.isnan(plane).all() and np.isnan(pixel).all() and plane.shape == (21,)


# ---- table scores against the dense restatement --------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_table_scores_equal_the_dense_formulation(seed):
    P = _pe()
    H, W = 12, 16
    na, nb = (3, 5) if seed % 2 else (6, 2)
    la, lb = R.random_labels(seed, na, H, W, block=3), R.random_labels(100 + seed, nb, H, W, block=2 + seed % 3)
    if seed == 4:
        lb[:] = 0                                                   # no detections
    if seed == 5:
        lb = la.clip(0, nb).astype(np.int32)
    gt, pred = R.random_depths(seed, H, W)
    T, S = R.tables(la, lb, na, nb, gt, pred)
    assert _close(P.segmentation_scores(T), R.dense_scores(la, lb, na, nb))
    plane, pixel = P.recall_curves(T, S)
    dplane, dpixel = R.dense_curves(la, lb, na, nb, gt, pred)
    assert _close(plane, dplane) and _close(pixel, dpixel)
    assert np.all(np.diff(plane) >= 0) and np.all(np.diff(pixel) >= 0)


# ---- curves -------------------------------------------------------------------------------------------------------------------------

def test_iou_is_strict_and_the_error_threshold_is_not():
    P = _pe()
    T = np.array([[0, 10], [10, 20]], np.int64)                      # a = b = 30, T = 20: IoU = 20 / (30 + 30 - 20) = 0.5 exactly
    S = np.zeros_like(T)
    plane, pixel = P.recall_curves(T, S)
    assert not plane.any() and not pixel.any()
    plane, _ = P.recall_curves(T, S, iou=0.4999)
    assert plane.all()
    T = np.array([[0, 9], [10, 20]], np.int64)                       # IoU = 20 / 39 > 0.5
    for k in (1, 2, 7, 20):                                          # D exactly on the threshold 0.05 k: matched there, not one threshold below
        t = P.THRESHOLDS[k]
        s = int(round(t * 20 * P.DEPTH_SCALE))
        while s / (20.0 * P.DEPTH_SCALE) > t:                        # the largest sum whose mean is <= t in fp64
            s -= 1
        while (s + 1) / (20.0 * P.DEPTH_SCALE) <= t:
            s += 1
        S = np.array([[0, 0], [0, s]], np.int64)
        plane, pixel = P.recall_curves(T, S)
        assert plane[k] == 1.0 and plane[k - 1] == 0.0 and pixel[k] == 20.0 / 30.0
        S[1, 1] += 1
        assert P.recall_curves(T, S)[0][k] == 0.0
    exact = P.recall_curves(T, np.array([[0, 0], [0, 20 * P.DEPTH_SCALE // 4]], np.int64), thresholds=[0.25, 0.2499])[0]      # D = 0.25 exactly
    assert exact.tolist() == [1.0, 0.0]
    # a ground-truth plane without pixels is a plane that is not recalled (its cells have D = 1e6); it adds nothing to the pixel recall
    T = np.array([[0, 0, 0], [0, 30, 0], [0, 0, 0]], np.int64)
    plane, pixel = P.recall_curves(T, np.zeros_like(T))
    assert plane.tolist() == [0.5] * 21 and pixel.tolist() == [1.0] * 21


# ---- the numpy path of label_map / overlap -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,n", [(1, 1, 1), (5, 7, 3), (9, 13, 0), (6, 11, 33)])
def test_label_map_host_path(h, w, n):
    P = _pe()
    for dtype in (bool, np.uint8):
        m = R.random_masks(h * 100 + n, n, h, w, dtype=dtype)
        if dtype is np.uint8 and m.size >= 2:
            m.reshape(-1)[:2] = (2, 255)
        t = torch.from_numpy(m)
        for priority in ("first", "last"):
            got = P.label_map(t, priority)
            assert got.dtype == torch.int32 and got.shape == (h, w)
            assert np.array_equal(got.numpy(), R.paint(m, priority)) and np.array_equal(R.paint_fast(m, priority), R.paint(m, priority))
    parts = [torch.from_numpy(R.random_masks(7, 2, 5, 7)), None, torch.zeros(0, 5, 7, dtype=torch.bool), torch.from_numpy(R.random_masks(8, 4, 5, 7))]
    batch = P.label_map(parts)
    assert batch.shape == (4, 5, 7) and not batch[1].any() and not batch[2].any()
    assert torch.equal(batch[0], P.label_map(parts[0])) and torch.equal(batch[3], P.label_map(parts[3]))
    with pytest.raises(RuntimeError, match="priority"):
        P.label_map(parts[0], "best")
    with pytest.raises(RuntimeError, match="None"):
        P.label_map([None, None])
    with pytest.raises(RuntimeError, match="bool / uint8"):
        P.label_map(torch.zeros(2, 5, 7))


def test_overlap_host_path():
    P = _pe()
    H, W, na, nb = 9, 13, 4, 6
    la, lb = R.random_labels(1, na, H, W, block=3), R.random_labels(2, nb, H, W, block=2)
    la[0, :3], lb[1, :3] = (-1, na + 1, 7), (nb + 1, -5, 0)          # dropped
    gt, pred = R.random_depths(3, H, W)
    gt[2, :4], pred[2, :4] = (5e-5, 0.0, 1.0, 1.0), (3.0, 3.0, np.nan, 5000.0)
    pred[3, 0] = np.inf
    count, wsum = P.overlap(torch.from_numpy(la), torch.from_numpy(lb), na, nb, torch.from_numpy(gt), torch.from_numpy(pred)[None])
    T, S = R.tables(la, lb, na, nb, gt, pred)
    assert count.dtype == torch.int64 and count.shape == (na + 1, nb + 1) and np.array_equal(count.numpy(), T) and np.array_equal(wsum.numpy(), S)
    assert int(T.sum()) == H * W - 5 and S.max() >= 1024 * 2 ** 20
    Tf, Sf = R.tables_fast(la, lb, na, nb, gt, pred)
    assert np.array_equal(Tf, T) and np.array_equal(Sf, S)
    c2, s2 = P.overlap(torch.from_numpy(np.stack([la, lb.clip(0, na)])), torch.from_numpy(np.stack([lb, la])), na, nb)
    assert c2.shape == (2, na + 1, nb + 1) and np.array_equal(c2[0].numpy(), T) and not s2.any()
    for bad in ((1024, 1), (1, -1), (True, 1), (1.0, 1)):
        with pytest.raises(RuntimeError, match="1023"):
            P.overlap(torch.from_numpy(la), torch.from_numpy(lb), *bad)
    with pytest.raises(RuntimeError, match="together"):
        P.overlap(torch.from_numpy(la), torch.from_numpy(lb), na, nb, torch.from_numpy(gt))
    with pytest.raises(RuntimeError, match="int32"):
        P.overlap(torch.from_numpy(la).long(), torch.from_numpy(lb), na, nb)


def test_quantisation_rule_on_the_host():
    """the ties of the rounding (e = k * 2^-21: half a unit), the cap, the non-finite values and the missing-ground-truth rule"""
    P = _pe()
    k = np.arange(0, 64, dtype=np.float32)
    e = k * np.float32(2.0 ** -21)
    gt = np.full(e.shape, 1.0, np.float32)
    pred = gt + e                                                    # exact in fp32: 1 + k 2^-21, k < 2^-2 / 2^-21
    assert np.array_equal(pred - gt, e)
    q = P._quantise_np(gt, pred)
    want = np.array([(int(v) // 2) + (int(v) % 2) * ((int(v) // 2) % 2) for v in k], np.int64)      # k / 2 rounded half to even
    assert np.array_equal(q, want) and np.array_equal(R.quantise(gt, pred).astype(np.int64), want)
    gt = np.array([1.0, 1.0, 1.0, 1.0, 0.0, 5e-5, 1e-4, np.nan], np.float32)
    pred = np.array([np.nan, np.inf, 2001.0, 1025.0, 9.0, 9.0, 1.0001, 1.0], np.float32)
    cap = 1024 * 2 ** 20
    q = P._quantise_np(gt, pred)
    assert q[:6].tolist() == [cap, cap, cap, cap, 0, 0]
    assert q[6] == int(np.rint(np.float32(np.float32(1.0001) - np.float32(1e-4)) * np.float32(2 ** 20))) and q[7] == cap
    assert np.array_equal(q, R.quantise(gt, pred).astype(np.int64))


def test_accumulator_on_the_host():
    P = _pe()
    H, W = 12, 16
    acc = P.PlaneEvalAccumulator()
    want = []
    for f, (ng, npred) in enumerate(((3, 4), (2, 0), (4, 2))):
        g, p = R.random_masks(f, ng, H, W), R.random_masks(50 + f, npred, H, W)
        gt, pred = R.random_depths(f, H, W)
        acc.add_frame(torch.from_numpy(g), torch.from_numpy(gt)[None], torch.from_numpy(p) if f != 1 else None, torch.from_numpy(pred)[None, None])
        la, lb = R.paint(g), R.paint(p)
        want.append((la, lb, ng, npred, gt, pred))
    tabs = acc.tables()
    scores, planes, pixels = [], [], []
    for (T, S), (la, lb, ng, npred, gt, pred) in zip(tabs, want):
        Tw, Sw = R.tables(la, lb, ng, npred, gt, pred)
        assert np.array_equal(T, Tw) and np.array_equal(S, Sw)
        scores.append(R.dense_scores(la, lb, ng, npred))
        pl, px = R.dense_curves(la, lb, ng, npred, gt, pred)
        planes.append(pl)
        pixels.append(px)
    res = acc.result()
    assert res["frames"] == 3 and res["curve_frames"] == 3 and len(acc) == 3
    assert _close([res["RI"], res["VOI"], res["SC"]], np.mean(scores, 0))
    assert _close(res["plane_recall"], np.mean(planes, 0)) and _close(res["pixel_recall"], np.mean(pixels, 0))
    empty = P.PlaneEvalAccumulator().result()
    assert math.isnan(empty["RI"]) and empty["frames"] == 0 and len(empty["plane_recall"]) == 21


def test_means_ignore_nan_frames():
    P = _pe()
    acc = P.PlaneEvalAccumulator()
    g = torch.zeros(1, 4, 4, dtype=torch.bool)
    g[0, :2] = True
    d = torch.ones(1, 4, 4)
    acc.add_frame(g, d, g, d)                                        # perfect
    acc.add_frame(torch.zeros(0, 4, 4, dtype=torch.bool), d, g, d)   # no ground-truth plane: NaN scores and curves, skipped
    res = acc.result()
    assert (res["RI"], res["VOI"], res["SC"]) == (1.0, 0.0, 1.0) and res["frames"] == 1 and res["curve_frames"] == 1
    assert res["plane_recall"] == [1.0] * 21 and res["pixel_recall"] == [1.0] * 21


def test_plane_metrics_flag_parses_and_defaults_to_off():
    import eval as ev
    assert ev.parse_args(["--no_bar"]).plane_metrics is False
    assert ev.parse_args(["--no_bar", "--plane_metrics"]).plane_metrics is True
    ev.parse_args(["--no_bar"])
