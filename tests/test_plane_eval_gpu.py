"""GPU: label maps and overlap tables on the device (planerecnet_amd/plane_eval.py, csrc/prn_plane_eval.hip) against the plain-numpy
restatement (tests/plane_eval_restate.py): image sizes round the 16-pixel thread and the vector loads' alignment, mask counts from none to a
hundred, both priorities, table sizes at and round the LDS limit, a full 480 x 640 frame, the depth values at which the fixed-point rule
decides, dropped labels, a ragged batch, no host synchronisation, refusals before any launch, the accumulator and eval.py's flag.  Every
device comparison is exact."""
import ctypes
import io
import math
import random
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import plane_eval_restate as R

pytestmark = pytest.mark.gpu

CAP = 1024 * 2 ** 20


def _pe():
    from planerecnet_amd import plane_eval
    return plane_eval


def _tables(P, la, lb, na, nb, gt=None, pred=None):
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    c, s = P.overlap(dev(la), dev(lb), na, nb, dev(gt), dev(pred))
    assert c.dtype == torch.int64 and s.dtype == torch.int64 and c.is_cuda and s.is_cuda
    return c.cpu().numpy(), s.cpu().numpy()


# ---- label_map ----------------------------------------------------------------------------------------------------------------------

SIZES = [(1, 1), (5, 7), (37, 65), (3, 63), (3, 64), (3, 65)]


@pytest.mark.parametrize("h,w", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_label_map_sizes_counts_priorities_dtypes(h, w):
    """an odd h * w puts most masks on an odd address, h * w = 192 every mask on a 16-byte boundary, 189 and 195 round it"""
    P = _pe()
    for n in (0, 1, 2, 33, 100):
        masks = R.random_masks(h * 1000 + w * 10 + n, n, h, w, fill=0.7)
        if n >= 2:
            masks[0] = True                                          # everything overlaps mask 0 ...
            masks[n - 1, h // 2:] = True                             # ... and the last mask in the lower half
        want = {p: R.paint(masks, p) for p in ("first", "last")}
        if n >= 2:
            assert (want["first"] == 1).all() and (want["last"][h // 2:] == n).all()
        weights = np.random.RandomState(n).randint(1, 256, masks.shape).astype(np.uint8)
        if masks.size >= 2:
            weights.reshape(-1)[:2] = (2, 255)
        for m in (torch.from_numpy(masks).cuda(), torch.from_numpy(masks * weights).cuda()):
            before = m.clone()
            for p in ("first", "last"):
                got = P.label_map(m, p)
                assert got.dtype == torch.int32 and got.shape == (h, w) and got.is_cuda
                assert np.array_equal(got.cpu().numpy(), want[p]), (n, p, str(m.dtype))
                both = P.label_map([None, m], p)                     # two images: the pointer-table launch (one image takes the flat one)
                assert both.shape == (2, h, w) and not both[0].any() and torch.equal(both[1], got), (n, p, str(m.dtype))
            assert torch.equal(m, before)
            if n >= 2 and h * w >= 2 and m.dtype == torch.uint8:
                assert m.view(-1)[:2].tolist() == [2, 255]           # (mask 0 is all set: its first bytes carry the two values)


def test_label_map_ragged_batch_equals_per_image_calls():
    P = _pe()
    H, W = 37, 65
    parts = [R.random_masks(40 + b, n, H, W) for b, n in enumerate((3, 0, 1, 5))]
    dev = [torch.from_numpy(p).cuda() for p in parts]
    masks = [dev[0], None, dev[1], dev[2], None, dev[3]]
    for p in ("first", "last"):
        batch = P.label_map(masks, p)
        assert batch.shape == (6, H, W) and batch.dtype == torch.int32
        for b, k in ((0, 0), (2, 1), (3, 2), (5, 3)):
            assert torch.equal(batch[b], P.label_map(dev[k], p)) and np.array_equal(batch[b].cpu().numpy(), R.paint(parts[k], p))
        assert not batch[1].any() and not batch[2].any() and not batch[4].any()
    wide = torch.zeros(5, H, W + 3, dtype=torch.bool).cuda()         # a non-contiguous view is read as what it shows
    wide[:, :, 3:] = dev[3]
    assert torch.equal(P.label_map(wide[:, :, 3:]), P.label_map(dev[3]))
    with pytest.raises(RuntimeError, match="one device, dtype and H x W"):
        P.label_map([dev[0], torch.zeros(1, H, W + 1, dtype=torch.bool).cuda()])


def test_label_map_480x640():
    P = _pe()
    masks = R.random_masks(5, 100, 480, 640, fill=0.4)
    dev = torch.from_numpy(masks).cuda()
    for p in ("first", "last"):
        assert np.array_equal(P.label_map(dev, p).cpu().numpy(), R.paint_fast(masks, p))


# ---- overlap ------------------------------------------------------------------------------------------------------------------------

def _limit_cases(P):
    side = math.isqrt(P.LDS_BINS)
    assert side * side == P.LDS_BINS and side == 64
    return [(side - 1, side - 1, 70, 130), (side - 1, side, 70, 130), (0, 0, 70, 130), (P.MAX_LABEL, P.MAX_LABEL, 5, 7)]


@pytest.mark.parametrize("case", range(4), ids=["lds-limit", "above-limit", "1x1", "1023x1023"])
def test_overlap_round_the_lds_limit(case):
    """(A + 1) * (B + 1) = LDS_BINS, just above it (the global-atomics path), one bin, and the largest table on a tiny image; 70 x 130
    pixels are three workgroups, the last one partly past the end"""
    P = _pe()
    na, nb, H, W = _limit_cases(P)[case]
    assert ((na + 1) * (nb + 1) <= P.LDS_BINS) == (case in (0, 2))
    rng = np.random.RandomState(case)
    la = np.stack([R.random_labels(case, na, H, W, block=2), rng.randint(0, na + 1, (H, W)).astype(np.int32)])
    lb = np.stack([R.random_labels(9 + case, nb, H, W, block=3), rng.randint(0, nb + 1, (H, W)).astype(np.int32)])
    la[0, 0, 0], lb[0, 0, 0], la[1, -1, -1], lb[1, -1, -1] = na, nb, na, nb                       # the last bin, first and last pixel
    gt, pred = (np.stack(x) for x in zip(R.random_depths(case, H, W), R.random_depths(case + 1, H, W)))
    T, S = _tables(P, la, lb, na, nb, gt, pred)
    assert T.shape == (2, na + 1, nb + 1)
    for b in range(2):
        Tw, Sw = R.tables_fast(la[b], lb[b], na, nb, gt[b], pred[b])
        assert np.array_equal(T[b], Tw) and np.array_equal(S[b], Sw) and T[b].sum() == H * W
    if H * W < 100:
        Tw, Sw = R.tables(la[0], lb[0], na, nb, gt[0], pred[0])
        assert np.array_equal(T[0], Tw) and np.array_equal(S[0], Sw)
    T0, S0 = _tables(P, la, lb, na, nb)                              # without depths: the same counts, no sums
    assert np.array_equal(T0, T) and not S0.any()


def test_overlap_small_against_the_dictionary():
    P = _pe()
    for h, w in SIZES:
        na, nb = 3, 4
        la, lb = R.random_labels(h, na, h, w, block=2), R.random_labels(w, nb, h, w, block=3)
        gt, pred = R.random_depths(h + w, h, w)
        T, S = _tables(P, la, lb, na, nb, gt, pred)
        Tw, Sw = R.tables(la, lb, na, nb, gt, pred)
        assert T.shape == (na + 1, nb + 1) and np.array_equal(T, Tw) and np.array_equal(S, Sw), (h, w)


def test_overlap_480x640():
    P = _pe()
    H, W = 480, 640
    la, lb = np.full((H, W), 3, np.int32), np.full((H, W), 5, np.int32)
    gt, pred = np.full((H, W), 2.0, np.float32), np.full((H, W), 2.3, np.float32)
    q = int(R.quantise(gt[:1, :1], pred[:1, :1])[0, 0])
    assert q == int(np.rint(np.float32(np.float32(2.3) - np.float32(2.0)) * np.float32(2 ** 20))) and q > 0
    T, S = _tables(P, la, lb, 20, 100, gt, pred)                     # every pixel in one bin: every thread adds to one LDS address
    assert T[3, 5] == 307200 and S[3, 5] == 307200 * q and T.sum() == 307200 and S.sum() == 307200 * q
    yy, xx = np.mgrid[:H, :W]
    la = (1 + (yy + xx) % 2).astype(np.int32)                        # a checkerboard: every run is one pixel long
    lb = (2 - (yy + xx) % 2).astype(np.int32)
    gt, pred = R.random_depths(1, H, W)
    T, S = _tables(P, la, lb, 2, 2, gt, pred)
    Tw, Sw = R.tables_fast(la, lb, 2, 2, gt, pred)
    assert np.array_equal(T, Tw) and np.array_equal(S, Sw) and T[1, 2] == 153600 and T[2, 1] == 153600
    T, S = _tables(P, la, lb, 63, 64, gt, pred)                      # the same through the global-atomics path
    assert np.array_equal(T[:3, :3], Tw) and np.array_equal(S[:3, :3], Sw) and T.sum() == 307200


def test_overlap_drops_labels_out_of_range():
    P = _pe()
    H, W, na, nb = 37, 65, 4, 6
    la, lb = R.random_labels(1, na, H, W), R.random_labels(2, nb, H, W)
    la[0, :4], lb[1, :4] = (-1, na + 1, 2 ** 31 - 1, -2 ** 31), (nb + 1, -7, 1 << 20, -1)
    la[5, 5], lb[5, 5] = -1, nb + 1                                  # both out of range: one dropped pixel
    gt, pred = R.random_depths(3, H, W)
    T, S = _tables(P, la, lb, na, nb, gt, pred)
    Tw, Sw = R.tables(la, lb, na, nb, gt, pred)
    assert np.array_equal(T, Tw) and np.array_equal(S, Sw) and T.sum() == H * W - 9
    T, _ = _tables(P, la, lb, P.MAX_LABEL, P.MAX_LABEL)              # the global path drops them too (na + 1 and nb + 1 are in range there)
    assert T.sum() == H * W - 7 and np.array_equal(T, R.tables_fast(la, lb, P.MAX_LABEL, P.MAX_LABEL)[0])


def test_overlap_depth_values():
    """NaN, inf and 2000 m score as 1024 m; e = k * 2^-21 are the ties of the rounding; depth_a of 0 and 5e-5 zero the term"""
    P = _pe()
    k = np.arange(64, dtype=np.float32)
    gt = np.ones(64, np.float32)
    pred = gt + k * np.float32(2.0 ** -21)
    assert np.array_equal(pred - gt, k * np.float32(2.0 ** -21))     # exact in fp32
    ties = np.array([(int(v) // 2) + (int(v) % 2) * ((int(v) // 2) % 2) for v in k], np.int64)      # k / 2, halves to even
    special_gt = np.array([1.0, 1.0, 1.0, 2001.0, 0.0, 5e-5, 1e-4, np.nan, -1.0, 3.0], np.float32)
    special_pred = np.array([np.nan, np.inf, 2001.0, 1.0, 7.0, 7.0, 1.0001, 1.0, 4.0, -np.inf], np.float32)
    special = np.array([CAP, CAP, CAP, CAP, 0, 0, -1, CAP, 0, CAP], np.int64)
    special[6] = int(np.rint(np.float32(np.float32(1.0001) - np.float32(1e-4)) * np.float32(2 ** 20)))
    gt, pred, want = np.concatenate([gt, special_gt]), np.concatenate([pred, special_pred]), np.concatenate([ties, special])
    assert np.array_equal(R.quantise(gt, pred).astype(np.int64), want)
    n = gt.size
    labels = np.arange(n, dtype=np.int32).reshape(1, n)              # one pixel per row of the table
    zeros = np.zeros((1, n), np.int32)
    for nb in (0, 63):                                               # the LDS and the global path
        T, S = _tables(P, labels, zeros, n - 1, nb, gt.reshape(1, n), pred.reshape(1, n))
        assert np.array_equal(T[:, 0], np.ones(n, np.int64)) and np.array_equal(S[:, 0], want) and not S[:, 1:].any()
    T, S = _tables(P, zeros, zeros, 0, 0, gt.reshape(1, n), pred.reshape(1, n))      # all in one bin: the sum of a run
    assert T[0, 0] == n and S[0, 0] == want.sum()


def test_overlap_two_runs_agree_and_a_batch_equals_per_image_calls():
    P = _pe()
    H, W, B = 70, 130, 3
    for na, nb in ((5, 7), (63, 64)):
        la = torch.from_numpy(np.stack([R.random_labels(b, na, H, W, block=1 + b) for b in range(B)])).cuda()
        lb = torch.from_numpy(np.stack([R.random_labels(9 + b, nb, H, W, block=2) for b in range(B)])).cuda()
        gt, pred = (torch.from_numpy(np.stack(x)).cuda() for x in zip(*[R.random_depths(b, H, W) for b in range(B)]))
        keep = [t.clone() for t in (la, lb, gt, pred)]
        first, second = P.overlap(la, lb, na, nb, gt, pred), P.overlap(la, lb, na, nb, gt, pred)
        assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
        for b in range(B):
            c, s = P.overlap(la[b], lb[b], na, nb, gt[b], pred[b])
            assert c.shape == (na + 1, nb + 1) and torch.equal(c, first[0][b]) and torch.equal(s, first[1][b])
        assert all(torch.equal(a, b) for a, b in zip(keep, (la, lb, gt, pred)))


def test_no_host_synchronisation():
    """Fails on a host implementation: that one downloads the maps."""
    P = _pe()
    H, W = 37, 65
    parts = [R.random_masks(b, n, H, W) for b, n in enumerate((3, 0, 5))]
    masks = [torch.from_numpy(p).cuda() for p in parts]
    gt, pred = (torch.from_numpy(x).cuda() for x in R.random_depths(1, H, W))
    la = P.label_map(masks)
    P.overlap(la[0], la[2], 3, 5, gt, pred), P.overlap(la, la, 63, 64)                     # warm: code objects loaded
    acc = P.PlaneEvalAccumulator()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda").item()                                             # the mode does catch a synchronisation
        la = P.label_map(masks)
        last = P.label_map(masks[2], "last")
        small = P.overlap(la[0], la[2], 3, 5, gt, pred)
        large = P.overlap(la, la, 63, 64)
        acc.add_frame(masks[0], gt, masks[2], pred)
        acc.add_frame(masks[2], gt, None, pred)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    wa, wb = R.paint(parts[0]), R.paint(parts[2])
    assert np.array_equal(la[0].cpu().numpy(), wa) and np.array_equal(la[2].cpu().numpy(), wb) and not la[1].any()
    assert np.array_equal(last.cpu().numpy(), R.paint(parts[2], "last"))
    Tw, Sw = R.tables(wa, wb, 3, 5, gt.cpu().numpy(), pred.cpu().numpy())
    assert np.array_equal(small[0].cpu().numpy(), Tw) and np.array_equal(small[1].cpu().numpy(), Sw)
    assert int(large[0].sum()) == 3 * H * W and int(large[0][0].diagonal().sum()) == H * W
    (T0, S0), (T1, S1) = acc.tables()
    assert np.array_equal(T0, Tw) and np.array_equal(S0, Sw) and T1.shape == (6, 1) and T1.sum() == H * W


def test_library_refuses_before_any_launch():
    """with real buffers: nothing is launched, the outputs keep their fill pattern"""
    from planerecnet_amd import _lib
    lib = _lib.lib
    H, W, A, B = 4, 6, 2, 3
    la = torch.ones(H, W, dtype=torch.int32).cuda()
    lb = torch.full((H, W), 2, dtype=torch.int32).cuda()
    d = torch.ones(H, W).cuda()
    count = torch.full(((A + 1) * (B + 1),), -7, dtype=torch.int64).cuda()
    wsum = torch.full(((A + 1) * (B + 1),), -7, dtype=torch.int64).cuda()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))

    def call(a=la, b=lb, da=d, db=d, n=1, h=H, w=W, na=A, nb=B, c=count, s=wsum):
        return lib.prn_label_overlap(p(a), p(b), p(da), p(db), n, h, w, na, nb, p(c), p(s), st)

    for kw, msg in ((dict(na=1024), b"1023"), (dict(nb=1024), b"1023"), (dict(na=-1), b"1023"), (dict(nb=-1), b"1023"),
                    (dict(h=4096, w=4096), b"2^24"), (dict(h=1 << 12, w=(1 << 12) + 1), b"2^24"), (dict(a=None), b"null label"),
                    (dict(b=None), b"null label"), (dict(da=None), b"go together"), (dict(db=None), b"go together"), (dict(c=None), b"null output"),
                    (dict(s=None), b"null output"), (dict(n=0), b"images"), (dict(h=0), b"H > 0")):
        assert call(**kw) != 0 and msg in lib.prn_last_error(), (kw, lib.prn_last_error())
    labels = torch.full((H * W,), -7, dtype=torch.int32).cuda()
    m = torch.ones(2, H, W, dtype=torch.uint8).cuda()
    ptrs = torch.tensor([m.data_ptr()], dtype=torch.int64).cuda()
    first = torch.tensor([0, 2], dtype=torch.int32).cuda()
    for args, msg in (((1, H, W, 2), b"priority"), ((0, H, W, 0), b"B <= 65535"), ((1, 1 << 16, 1 << 15, 0), b"2^31"), ((1, H, 0, 0), b"W > 0")):
        assert lib.prn_label_map(p(ptrs), p(first), *args, p(labels), st) != 0 and msg in lib.prn_last_error(), args
    assert lib.prn_label_map(None, p(first), 1, H, W, 0, p(labels), st) != 0 and b"null" in lib.prn_last_error()
    for args, msg in (((2, H, W, 2), b"priority"), ((0, H, W, 0), b"N >= 1"), ((2, 1 << 16, 1 << 15, 0), b"2^31"), ((2, 0, W, 0), b"H > 0")):
        assert lib.prn_label_map_flat(p(m), *args, p(labels), st) != 0 and msg in lib.prn_last_error(), args
    assert lib.prn_label_map_flat(None, 2, H, W, 0, p(labels), st) != 0 and b"null" in lib.prn_last_error()
    torch.cuda.synchronize()
    assert int((count != -7).sum()) == 0 and int((wsum != -7).sum()) == 0 and int((labels != -7).sum()) == 0
    count.zero_(), wsum.zero_()
    d2 = d * 1.5
    assert call(db=d2) == 0 and lib.prn_label_map(p(ptrs), p(first), 1, H, W, 1, p(labels), st) == 0
    want = torch.zeros(A + 1, B + 1, dtype=torch.int64)
    want[1, 2] = H * W
    assert torch.equal(count.cpu().view(A + 1, B + 1), want) and torch.equal(wsum.cpu().view(A + 1, B + 1), want * 2 ** 19)
    assert labels.tolist() == [2] * (H * W)
    assert lib.prn_label_map_flat(p(m), 2, H, W, 0, p(labels), st) == 0 and labels.tolist() == [1] * (H * W)
    P = _pe()
    with pytest.raises(RuntimeError, match="2\\^24"):
        P.overlap(torch.zeros(4096, 4096, dtype=torch.int32).cuda(), torch.zeros(4096, 4096, dtype=torch.int32).cuda(), 1, 1)


# ---- the accumulator and eval.py ---------------------------------------------------------------------------------------------------

def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and not np.isnan(a).any() and bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


def _frames(H=37, W=65):
    """three frames, the second without detections: (gt masks, pred masks, gt depth, pred depth) in numpy"""
    out = []
    for f, (ng, npred) in enumerate(((4, 5), (3, 0), (5, 3))):
        g = R.random_masks(f, ng, H, W)
        p = np.roll(g, 2, axis=2)[:npred] if npred else np.zeros((0, H, W), bool)       # detections: the planes shifted by two pixels
        if npred > ng - 1:
            p = np.concatenate([p, R.random_masks(70 + f, npred - len(p), H, W)])
        gt, pred = R.random_depths(f, H, W)
        out.append((g, p, gt, (gt + 0.05 * (f + 1) + 0.01 * np.random.RandomState(f).rand(H, W)).astype(np.float32) if f else pred))
    return out


def _restated(frames):
    tabs, scores, planes, pixels = [], [], [], []
    for g, p, gt, pred in frames:
        la, lb = R.paint_fast(g), R.paint_fast(p) if len(p) else np.zeros(g.shape[1:], np.int32)
        tabs.append(R.tables_fast(la, lb, len(g), len(p), gt, pred))
        scores.append(R.dense_scores(la, lb, len(g), len(p)))
        pl, px = R.dense_curves(la, lb, len(g), len(p), gt, pred)
        planes.append(pl)
        pixels.append(px)
    return tabs, np.mean(scores, 0), np.mean(planes, 0), np.mean(pixels, 0)


def test_accumulator_equals_the_restatement():
    P = _pe()
    frames = _frames()
    acc = P.PlaneEvalAccumulator()
    for f, (g, p, gt, pred) in enumerate(frames):
        pm = None if f == 1 else torch.from_numpy(p).cuda()
        acc.add_frame(torch.from_numpy(g).cuda(), torch.from_numpy(gt).cuda()[None], pm, torch.from_numpy(pred).cuda()[None, None])
    tabs, scores, planes, pixels = _restated(frames)
    for (T, S), (Tw, Sw) in zip(acc.tables(), tabs):
        assert np.array_equal(T, Tw) and np.array_equal(S, Sw)
    res = acc.result()
    assert res["frames"] == 3 and res["curve_frames"] == 3
    assert _close([res["RI"], res["VOI"], res["SC"]], scores) and _close(res["plane_recall"], planes) and _close(res["pixel_recall"], pixels)
    assert 0.0 < res["plane_recall"][-1] < 1.0 and res["plane_recall"][0] == 0.0      # the shifted planes are found, the frame without detections is not


class _StubNet(torch.nn.Module):
    """returns a prepared eval-mode result for the frame whose first pixel the image carries"""

    def __init__(self, results):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.results = results

    def forward(self, x):
        return [self.results[float(x[0, 0, 0, 0].item())]]


def test_evaluate_end_to_end():
    import eval as ev
    from planerecnet_amd import metrics
    from planerecnet_amd.datasets import SyntheticPlaneDataset
    dataset = SyntheticPlaneDataset(3, hw=(96, 128))
    results, frames = {}, []
    for i in range(3):
        image, inst, depth = dataset.pull_item(i)
        g = inst["masks"].numpy() != 0
        d = np.roll(g, 3, axis=2)[:len(g) - i]                       # the planes three pixels off; frame i misses its last i planes
        pred_depth = depth * 1.02 + 0.01 * i
        dm = torch.from_numpy(d).cuda()
        results[float(image[0, 0, 0])] = {"pred_masks": dm, "pred_boxes": metrics.mask_boxes(dm).cpu(), "pred_classes": torch.zeros(len(d)).cuda(),
                                          "pred_scores": torch.linspace(0.9, 0.5, len(d)).cuda(), "pred_depth": pred_depth.cuda()[None]}
        frames.append((g, d, depth[0].numpy(), pred_depth[0].numpy()))
    net = _StubNet(results).cuda()
    ev.parse_args(["--no_bar"])
    with torch.no_grad():
        random.seed(0)
        buf = io.StringIO()
        with redirect_stdout(buf):
            table, got = ev.evaluate(net, dataset, eval_nums=3, plane_metrics=True)
        random.seed(0)
        plain_buf = io.StringIO()
        with redirect_stdout(plain_buf):
            plain_table, plain = ev.evaluate(net, dataset, eval_nums=3)
    assert list(plain) == list(metrics.depth_metrics) and plain_table == table and list(table) == ["box", "mask"]
    assert list(got) == list(metrics.depth_metrics) + ["RI", "VOI", "SC", "plane_recall", "pixel_recall"]
    assert all(got[k] == plain[k] for k in plain)
    assert all(math.isfinite(got[k]) for k in ("RI", "VOI", "SC")) and 0.0 < got["RI"] <= 1.0 and got["VOI"] >= 0.0 and 0.0 < got["SC"] <= 1.0
    for k in ("plane_recall", "pixel_recall"):
        assert len(got[k]) == 21 and all(b >= a for a, b in zip(got[k], got[k][1:])) and 0.0 <= got[k][0] and 0.0 < got[k][-1] <= 1.0
    _, scores, planes, pixels = _restated(frames)
    assert _close([got["RI"], got["VOI"], got["SC"]], scores) and _close(got["plane_recall"], planes) and _close(got["pixel_recall"], pixels)
    text = buf.getvalue()
    assert "Plane segmentation: RI: %.5f, VOI: %.5f, SC: %.5f" % (got["RI"], got["VOI"], got["SC"]) in text
    rows = [ln for ln in text.splitlines() if ln.startswith(("depth m |", "  plane |", "  pixel |"))]
    assert len(rows) == 3 and all(len(r.split("|")[1].split()) == 20 for r in rows)
    assert "Plane segmentation" not in plain_buf.getvalue()
    extra = [ln for ln in text.splitlines() if ln not in plain_buf.getvalue().splitlines()]
    assert len(extra) == 4                                           # the flag adds its four lines and changes none
