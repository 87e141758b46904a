"""GPU: one reading rule for byte masks (planerecnet_amd/csrc/prn_masks.h).  The same uint8 masks -- bytes that are neither 0 nor 1 among
them -- go through every public entry that accepts uint8 masks, and every result must equal the numpy statement computed from `m != 0`.

Values   drawn by a seeded generator from {0, 0, 0, 1, 2, 0x10, 0x80, 0xff}.
Shapes   three masks per tensor, so that an odd H * W puts the second mask on an odd address: a row shorter than any vector (3 x 5), rows one
         below / at / one above a 64-bit word (7 x 63, 5 x 64, 9 x 65), a fully aligned case (4 x 16), a multi-word row with a tail (33 x 130).
Inputs   the three masks as a tensor of their own, and as a view one mask into a larger allocation (the base address is not the allocation's).
         Both live in int32 allocations, which the suite's guard mode (PRN_TEST_GUARD=1) brackets with non-zero bytes: a read past a mask then
         shows as set bits in a compared result.
Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import components_restate
import mask_nms_restate
import render_restate
import rle_restate

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5), (7, 63), (5, 64), (9, 65), (4, 16), (33, 130)]
VALUES = np.array([0, 0, 0, 1, 2, 0x10, 0x80, 0xff], np.uint8)
N = 3
shapes = pytest.mark.parametrize("h,w", SHAPES, ids=["%dx%d" % s for s in SHAPES])


@functools.lru_cache(maxsize=None)
def _host(h, w):
    """(bytes uint8 [N,h,w], set bool [N,h,w]) of a shape, computed once and never written"""
    rng = np.random.RandomState(1000 * h + w)
    m = VALUES[rng.randint(0, len(VALUES), size=(N, h, w))]
    s = m != 0
    assert s.any(axis=(1, 2)).all() and not s.all(axis=(1, 2)).any() and (m > 1).any()
    m.setflags(write=False)
    s.setflags(write=False)
    return m, s


def _device_bytes(host):
    """host uint8 array -> device tensor inside an int32 allocation; the bytes that round the allocation up are non-zero"""
    n = host.size
    buf = torch.empty((n + 3) // 4, dtype=torch.int32, device="cuda").view(torch.uint8)
    buf.fill_(0xff)
    buf[:n].copy_(torch.from_numpy(host.reshape(-1).copy()))
    return buf[:n].view(host.shape)


def _inputs(h, w):
    """the masks of a shape on the device, twice: [("own", tensor), ("view", a view offset by one mask into a larger allocation)]"""
    m, _ = _host(h, w)
    lead = np.full((1, h, w), 0xff, np.uint8)
    view = _device_bytes(np.concatenate([lead, m]))[1:]
    assert view.is_contiguous() and view.storage_offset() > 0
    return [("own", _device_bytes(m)), ("view", view)]


def _iou_reference(sa, sb):
    """fp32 [A,B]: intersection / ((area_a + area_b) - intersection), the kernel's operation order on exact integers"""
    a, b = sa.reshape(len(sa), -1), sb.reshape(len(sb), -1)
    inter = (a[:, None, :] & b[None, :, :]).sum(-1).astype(np.float32)
    aa, ab = a.sum(1).astype(np.float32), b.sum(1).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return inter / ((aa[:, None] + ab[None, :]) - inter)


@shapes
def test_pairwise_and_boundary_iou(h, w):
    """against the masks themselves, an empty mask and a full one (IoU = area / (h w): the packed areas), from both IoU entries"""
    from planerecnet_amd import metrics
    m, s = _host(h, w)
    others = np.concatenate([m, np.zeros((1, h, w), np.uint8), np.full((1, h, w), 0x80, np.uint8)])
    want = _iou_reference(s, others != 0)
    assert (want[np.arange(N), np.arange(N)] == 1).all() and (want[:, N] == 0).all()
    bs = [_device_bytes(np.concatenate([others[-1:], others]))[1:], _device_bytes(others)]
    for (tag, a), b in zip(_inputs(h, w), bs):                            # (own, view) and (view, own)
        got = metrics.pairwise_iou(masks_a=a, masks_b=b)[0]
        assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), tag
        got = metrics.boundary_iou(a, b, radius=1)[0]
        assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), tag


@shapes
def test_erode_radius_zero(h, w):
    from planerecnet_amd import morphology
    _, s = _host(h, w)
    ins = _inputs(h, w)
    for tag, a in ins:
        out, area = morphology.erode(a, radius=0, return_area=True)
        assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), s.astype(np.uint8)), tag
        assert np.array_equal(area.cpu().numpy(), s.reshape(N, -1).sum(1)), tag
    for out in morphology.erode([a for _, a in ins], radius=0):          # a ragged batch: the second image's masks are found by the search
        assert np.array_equal(out.cpu().numpy(), s.astype(np.uint8))


@shapes
def test_label(h, w):
    from planerecnet_amd import components
    _, s = _host(h, w)
    want, count = components_restate.label_flood_batch(s)
    ins = _inputs(h, w)
    for tag, a in ins:
        lab, cnt = components.label(a)
        assert np.array_equal(lab.cpu().numpy(), want) and np.array_equal(cnt.cpu().numpy(), count), tag
    for lab in components.label([a for _, a in ins])[0]:
        assert np.array_equal(lab.cpu().numpy(), want)


@shapes
def test_rle_encode_decode(h, w):
    from planerecnet_amd import rle
    _, s = _host(h, w)
    want = [rle_restate.counts_to_string(rle_restate.mask_to_counts(x)) for x in s]
    ins = _inputs(h, w)
    for tag, a in ins:
        got = rle.encode(a)
        assert [r["counts"] for r in got] == want and all(r["size"] == [h, w] for r in got), tag
        assert np.array_equal(rle.decode(got, "cuda").cpu().numpy(), s.astype(np.uint8)), tag
    assert [[r["counts"] for r in part] for part in rle.encode([a for _, a in ins])] == [want, want]


@shapes
def test_mask_nms(h, w):
    """the threshold sits exactly on the fp32 IoU of masks 0 and 1 (not above it: kept) and one step below it (suppressed), so one misread
    pixel of their intersection changes the answer"""
    from planerecnet_amd import nms
    _, s = _host(h, w)
    labels = np.zeros(N, np.int64)
    sums = s.reshape(N, -1).sum(1).astype(np.float32)
    tie = _iou_reference(s[:1], s[1:2])[0, 0]
    for thr in (float(tie), float(np.nextafter(tie, np.float32(0)))):
        want = mask_nms_restate.reference_loop(labels, s, sums, thr)
        for tag, a in _inputs(h, w):
            keep = nms.mask_nms_batched(torch.from_numpy(labels).cuda(), a, torch.from_numpy(sums).cuda(), [N], nms_thr=thr)
            assert keep.dtype == torch.uint8 and np.array_equal(keep.cpu().numpy(), want), (tag, thr)
    assert want[1] == 0 and mask_nms_restate.reference_loop(labels, s, sums, float(tie))[1] == 1


@shapes
def test_plane_pixel_counts(h, w):
    from planerecnet_amd import planes
    _, s = _host(h, w)
    depth = torch.full((1, 1, h, w), 2.0, device="cuda")
    k = np.array([[50.0, 0.0, w / 2], [0.0, 50.0, h / 2], [0.0, 0.0, 1.0]])
    for tag, a in _inputs(h, w):
        _, _, count = planes.fit_planes(depth, [a], k)
        assert np.array_equal(count[0].cpu().numpy(), s.reshape(N, -1).sum(1)), tag


@shapes
def test_overlay(h, w):
    """both mask readers of the renderer: four bytes per thread (no outlines) and the staged tiles (outlines)"""
    from planerecnet_amd import render
    m, _ = _host(h, w)
    frame = (np.random.RandomState(h + w).rand(h, w, 3) * 255).astype(np.float32)
    boxes = np.zeros((N, 4), np.float32)
    for contours in (False, True):
        want = render_restate.overlay(frame, m, boxes, no_box=True, contours=contours)
        for tag, a in _inputs(h, w):
            result = {"pred_masks": a, "pred_boxes": torch.from_numpy(boxes), "pred_scores": torch.ones(N)}
            got = render.render_overlay(result, torch.from_numpy(frame).cuda(), no_box=True, contours=contours)
            assert np.array_equal(got.cpu().numpy(), want), (tag, contours)
