"""GPU: the COCO run-length codec on the device (planerecnet_amd/rle.py, csrc/prn_rle.hip) against the hand-derived vectors
(tests/golden/coco_rle_vectors.json) and the loop-by-loop restatement (tests/rle_restate.py), and eval.py's detection files.  Every check
is `torch.equal` or string equality: the codec is integer arithmetic.

The shapes put W on and off the four-columns-per-lane path (W % 4), H across the 32-row segment edge (37, 65, 130, 480), more than one
workgroup per mask in x and in y, set runs across column boundaries, tiles of the painter with more run ends than its LDS stages (0.5
density at 65x257 and 130x515) and five-character counts (1030x1030)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rle_restate as R
from rle_restate import build_mask, load_vectors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def restate(mask):
    return R.counts_to_string(R.mask_to_counts(mask))


def shapes_mask(H, W, rng, n=4):
    """a detection-like mask: the union of rectangles and ellipses"""
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), bool)
    for i in range(n):
        h, w = max(1, int(H * rng.uniform(0.1, 0.5))), max(1, int(W * rng.uniform(0.1, 0.5)))
        y0, x0 = rng.randint(0, H - h + 1), rng.randint(0, W - w + 1)
        if i % 2:
            m |= ((yy - y0 - h / 2) / (h / 2)) ** 2 + ((xx - x0 - w / 2) / (w / 2)) ** 2 <= 1
        else:
            m[y0:y0 + h, x0:x0 + w] = True
    return m


def check_roundtrip(masks_np, masks_dev=None):
    """encode == the restatement, string for string; decode(encode(m)) == (m != 0)"""
    from planerecnet_amd import rle
    dev = torch.from_numpy(masks_np).to(DEV) if masks_dev is None else masks_dev
    got = rle.encode(dev)
    H, W = masks_np.shape[1:]
    assert len(got) == len(masks_np)
    for i, g in enumerate(got):
        assert g["size"] == [H, W] and g["counts"] == restate(masks_np[i]), (i, masks_np.shape)
    back = rle.decode(got, DEV)
    assert back.dtype == torch.uint8 and back.device == dev.device
    assert torch.equal(back, torch.from_numpy((masks_np != 0).astype(np.uint8)).to(DEV))
    return got


def test_fixture_vectors_encode_and_decode():
    from planerecnet_amd import rle
    for e in load_vectors()["masks"]:
        H, W = e["size"]
        m = build_mask(e["size"], e["mask"]) if "mask" in e else R.counts_to_mask(e["counts"], H, W)
        dev = torch.from_numpy(m).to(DEV)
        got = rle.encode(dev[None])
        assert got == [{"size": [H, W], "counts": e["string"]}], e["name"]
        for form in (e["string"], e["string"].encode("ascii"), e["counts"]):
            assert torch.equal(rle.decode([{"size": [H, W], "counts": form}], DEV)[0], dev), e["name"]
        assert rle.area(got[0]) == int(m.sum())


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (3, 4), (37, 53), (64, 256), (65, 257), (130, 515)])
def test_random_masks_equal_the_restatement(H, W):
    rng = np.random.RandomState(H * 1000 + W)
    masks = [rng.rand(H, W) < d for d in (0.0, 0.02, 0.5, 0.98, 1.0)] + [shapes_mask(H, W, rng)]
    check_roundtrip(np.stack(masks).astype(np.uint8))


def test_frame_sized_masks_equal_the_restatement():
    rng = np.random.RandomState(480640)
    masks = [rng.rand(480, 640) < 0.02, rng.rand(480, 640) < 0.5, shapes_mask(480, 640, rng, n=6)]
    check_roundtrip(np.stack(masks).astype(np.uint8))


def test_checkerboards_every_pixel_a_boundary():
    for H, W in ((5, 7), (37, 53)):
        yy, xx = np.mgrid[:H, :W]
        m = ((xx + yy) & 1).astype(np.uint8)
        got = check_roundtrip(np.stack([m, 1 - m]))
        assert got[0]["counts"] == "111" + "0" * (H * W - 3) and got[1]["counts"] == "011" + "0" * (H * W - 2)


def test_bool_and_byte_values_give_the_same_strings():
    from planerecnet_amd import rle
    rng = np.random.RandomState(5)
    b = np.stack([rng.rand(37, 52) < 0.4, shapes_mask(37, 52, rng)])
    values = np.array([1, 2, 255], np.uint8)[rng.randint(0, 3, size=b.shape)]
    as_bool = rle.encode(torch.from_numpy(b).to(DEV))
    as_bytes = rle.encode(torch.from_numpy(np.where(b, values, 0).astype(np.uint8)).to(DEV))
    assert as_bool == as_bytes and [g["counts"] for g in as_bool] == [restate(m) for m in b]
    assert torch.equal(rle.decode(as_bytes, DEV), torch.from_numpy(b.astype(np.uint8)).to(DEV))


def test_views_sliced_and_misaligned():
    from planerecnet_amd import rle
    rng = np.random.RandomState(6)
    big = torch.from_numpy((rng.rand(4, 70, 140) < 0.3).astype(np.uint8)).to(DEV)
    view = big[1:4, 3:67, 5:133]                               # [3,64,128]: W % 4 == 0, rows 140 bytes apart
    assert not view.is_contiguous()
    want = [restate(m) for m in view.cpu().numpy()]
    assert [g["counts"] for g in rle.encode(view)] == want
    assert [g["counts"] for g in rle.encode(view.contiguous())] == want
    flat = torch.zeros(3 * 64 * 128 + 1, dtype=torch.uint8, device=DEV)
    odd = flat[1:].view(3, 64, 128)                            # contiguous, one byte off every alignment: the byte-load form of the wide path
    odd.copy_(view)
    assert odd.is_contiguous() and odd.data_ptr() % 4 != 0
    assert [g["counts"] for g in rle.encode(odd)] == want
    assert torch.equal(rle.decode(rle.encode(odd), DEV), view.contiguous())


def test_ragged_list_equals_per_image_calls():
    from planerecnet_amd import rle
    rng = np.random.RandomState(7)
    a = torch.from_numpy((rng.rand(2, 37, 53) < 0.3)).to(DEV)
    c = torch.from_numpy((rng.rand(5, 37, 53) < 0.6).astype(np.uint8)).to(DEV)
    empty = torch.zeros(0, 37, 53, dtype=torch.bool, device=DEV)
    got = rle.encode([a, empty, c])
    assert [len(g) for g in got] == [2, 0, 5]
    assert got[0] == rle.encode(a) and got[2] == rle.encode(c) and got[1] == []
    assert rle.encode([a, None, c]) == got and rle.encode([None, a]) == [[], got[0]]
    assert rle.encode(empty) == [] and rle.encode([empty, None]) == [[], []] and rle.encode([]) == []
    assert [g["counts"] for g in got[0] + got[2]] == [restate(m) for m in list(a.cpu().numpy()) + list(c.cpu().numpy())]
    assert torch.equal(rle.decode(got[0] + got[2], DEV), torch.cat([a.to(torch.uint8), c]))


def test_decode_uncompressed_and_leading_zero_count():
    from planerecnet_amd import rle
    m = np.zeros((4, 5), np.uint8)
    m[1:3, 1:4] = 1
    lead = np.ones((3, 4), np.uint8)
    lead[2, 3] = 0
    out = rle.decode([{"size": [4, 5], "counts": [5, 2, 2, 2, 2, 2, 5]}, {"size": [4, 5], "counts": [0, 20]}, {"size": [4, 5], "counts": [20]}], DEV)
    assert torch.equal(out, torch.from_numpy(np.stack([m, np.ones_like(m), np.zeros_like(m)])).to(DEV))
    out = rle.decode([{"size": [3, 4], "counts": [0, 11, 1]}, {"size": [3, 4], "counts": "0;1"}, {"size": [3, 4], "counts": [0, 0, 0, 11, 1]}], DEV)
    assert torch.equal(out, torch.from_numpy(np.stack([lead, lead, lead])).to(DEV))
    assert R.counts_to_string([0, 11, 1]) == "0;1" and np.array_equal(R.counts_to_mask([0, 0, 0, 11, 1], 3, 4), lead)


def test_two_calls_give_identical_results():
    from planerecnet_amd import rle
    rng = np.random.RandomState(8)
    m = torch.from_numpy(np.stack([rng.rand(130, 516) < 0.5, shapes_mask(130, 516, rng)])).to(DEV)
    first, second = rle.encode(m), rle.encode(m)
    assert first == second
    assert torch.equal(rle.decode(first, DEV), rle.decode(second, DEV))


def test_collector_on_a_synthetic_result():
    """one result dict as the model returns it (masks and scores on the device, boxes on the host) through eval.py's collector and JSON"""
    import eval as ev
    from planerecnet_amd import rle
    rng = np.random.RandomState(9)
    masks = np.stack([shapes_mask(96, 128, rng) for _ in range(4)])
    boxes = torch.tensor(rng.uniform(0, 90, size=(4, 2)).tolist()).repeat(1, 2) + torch.tensor([0.0, 0.0, 17.37, 30.04])
    result = {"pred_masks": torch.from_numpy(masks).to(DEV), "pred_boxes": boxes.float(), "pred_classes": torch.zeros(4, dtype=torch.int64, device=DEV),
              "pred_scores": torch.linspace(0.9, 0.3, 4).to(DEV), "pred_depth": None}
    det = ev.Detections()
    det.add_frame(3, result, {1: 1})
    bbox, mask = json.loads(json.dumps([det.bbox_data, det.mask_data]))
    assert len(bbox) == len(mask) == 4
    for i in range(4):
        x0, y0, x1, y1 = result["pred_boxes"][i].tolist()
        assert bbox[i] == {"image_id": 3, "category_id": 1, "bbox": [round(float(v) * 10) / 10 for v in (x0, y0, x1 - x0, y1 - y0)],
                           "score": float(result["pred_scores"][i])}
        assert mask[i]["image_id"] == 3 and mask[i]["category_id"] == 1 and mask[i]["score"] == bbox[i]["score"]
        assert mask[i]["segmentation"]["counts"] == restate(masks[i])
        assert torch.equal(rle.decode([mask[i]["segmentation"]], DEV)[0], result["pred_masks"][i].to(torch.uint8))


def test_eval_writes_detection_files(tmp_path):
    from planerecnet_amd import rle
    bbox_file, mask_file = os.path.join(tmp_path, "out", "bbox.json"), os.path.join(tmp_path, "out", "mask.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py"), "--config", "PlaneRecNet_50_config", "--dataset", "synthetic", "--max_images", "3",
                        "--synthetic_size", "4", "--score_threshold", "0.05", "--no_bar", "--output_coco_json", "--bbox_det_file", bbox_file,
                        "--mask_det_file", mask_file], cwd=str(tmp_path), capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
    with open(bbox_file) as f:
        bbox = json.load(f)
    with open(mask_file) as f:
        mask = json.load(f)
    assert isinstance(bbox, list) and isinstance(mask, list) and len(bbox) == len(mask)      # (may be empty with random weights)
    print("eval.py wrote %d detections" % len(bbox))
    for b, m in zip(bbox, mask):
        assert sorted(b) == ["bbox", "category_id", "image_id", "score"] and len(b["bbox"]) == 4
        assert m["image_id"] == b["image_id"] and m["segmentation"]["size"] == [480, 640]
    if mask:
        out = rle.decode([m["segmentation"] for m in mask], DEV)
        assert tuple(out.shape) == (len(mask), 480, 640)
        assert [int(v) for v in out.flatten(1).sum(1).tolist()] == [rle.area(m["segmentation"]) for m in mask]
