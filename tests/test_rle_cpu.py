"""CPU: the COCO run-length format on the host -- the loop-by-loop restatement (tests/rle_restate.py) against the hand-derived vectors of
tests/golden/coco_rle_vectors.json, planerecnet_amd.rle's vectorised host helpers against the restatement, decode()'s input validation
(before any device use) and the layout of eval.py's Detections entries.  Everything is integer or string equality."""
import json
import os

import numpy as np
import pytest

import rle_restate as R
from rle_restate import build_mask, load_vectors

def random_count_lists(n=200, seed=0):
    """seeded count lists: lengths 1 .. 40, magnitudes from single pixels to 2^31 - 1, and -- in every list of four counts or more -- one
    difference to count i-2 planted at an edge of the character-length rule"""
    rng = np.random.RandomState(seed)
    edges = [-513, -512, -17, -16, -1, 0, 15, 16, 511, 512]
    top = (1 << 31) - 1
    lists = []
    for t in range(n):
        hi = [2, 40, 1100, 1 << 20, top][t % 5]
        c = [int(v) for v in rng.randint(0, hi, size=rng.randint(1, 41), dtype=np.int64)]
        if len(c) >= 4:
            i = int(rng.randint(3, len(c)))
            d = edges[t % len(edges)]
            c[i - 2] = max(c[i - 2], 600)
            c[i] = c[i - 2] + d
        if t % 17 == 0:
            c[int(rng.randint(0, len(c)))] = top
        lists.append(c)
    return lists


def test_restatement_reproduces_every_vector():
    v = load_vectors()
    assert len(v["masks"]) == 15 and len(v["deltas"]["cases"]) == 12
    for e in v["masks"]:
        H, W = e["size"]
        assert sum(e["counts"]) == H * W, e["name"]
        assert R.counts_to_string(e["counts"]) == e["string"], e["name"]
        assert R.string_to_counts(e["string"]) == e["counts"], e["name"]
        if "mask" in e:
            m = build_mask(e["size"], e["mask"])
            assert R.mask_to_counts(m) == e["counts"], e["name"]
            assert np.array_equal(R.counts_to_mask(e["counts"], H, W), m), e["name"]
            assert R.area(e["counts"]) == int(m.sum()), e["name"]
    for d in v["deltas"]["cases"]:
        assert R.counts_to_string([0, 0, 0, d["x"]]) == "000" + d["chars"], d
        assert R.string_to_counts("000" + d["chars"]) == [0, 0, 0, d["x"]], d


def test_host_helpers_equal_the_restatement_on_the_vectors():
    from planerecnet_amd import rle
    v = load_vectors()
    for e in v["masks"]:
        assert rle.counts_to_string(e["counts"]) == e["string"], e["name"]
        assert rle.string_to_counts(e["string"]).tolist() == e["counts"], e["name"]
        assert rle.string_to_counts(e["string"].encode("ascii")).tolist() == e["counts"], e["name"]
        for form in (e["string"], e["string"].encode("ascii"), e["counts"]):
            assert rle.area({"size": e["size"], "counts": form}) == R.area(e["counts"]), e["name"]
    for d in v["deltas"]["cases"]:                           # as real counts: [0, 600, 0, 600 + x] has x as its fourth difference
        c = [0, 600, 0, 600 + d["x"]]
        s = rle.counts_to_string(c)
        assert s == R.counts_to_string(c) and s.endswith("0" + d["chars"]) and rle.string_to_counts(s).tolist() == c, d
    assert rle.counts_to_string([]) == "" and rle.string_to_counts("").tolist() == []


def test_host_helpers_equal_the_restatement_on_random_counts():
    from planerecnet_amd import rle
    lists = random_count_lists()
    assert len(lists) == 200
    seen = set()
    for c in lists:
        s = R.counts_to_string(c)
        assert rle.counts_to_string(c) == s, c
        assert rle.string_to_counts(s).tolist() == c == R.string_to_counts(s), c
        assert rle.area({"size": [1, sum(c)], "counts": s}) == R.area(c) == rle.area({"size": [1, sum(c)], "counts": c}), c
        seen.update(c[i] - c[i - 2] for i in range(3, len(c)))
    assert {-513, -512, -17, -16, -1, 0, 15, 16, 511, 512} <= seen and max(max(c) for c in lists) == (1 << 31) - 1


def test_decode_refuses_bad_input_before_any_device_use(monkeypatch):
    """the three input faults raise ValueError on a machine without a GPU: nothing is uploaded, allocated or launched before them"""
    import torch
    from planerecnet_amd import rle

    def no_device(*a, **k):
        raise AssertionError("decode touched the device before validating its input")
    monkeypatch.setattr(rle.lib, "prn_rle_paint", no_device, raising=False)
    monkeypatch.setattr(torch, "empty", no_device)
    monkeypatch.setattr(rle, "_upload", no_device)
    good = R.counts_to_string([5, 2, 2, 2, 2, 2, 5])
    assert rle.string_to_counts(good).sum() == 20
    with pytest.raises(ValueError, match="negative"):
        rle.decode([{"size": [4, 5], "counts": [5, -2, 17]}], "cuda:0")
    with pytest.raises(ValueError, match="negative"):                                        # a string that decodes to a negative count
        rle.decode([{"size": [4, 5], "counts": R.counts_to_string([5, 2, 2]) + R.counts_to_string([0, 0, 0, -3])[3:]}], "cuda:0")
    with pytest.raises(ValueError, match="sum"):
        rle.decode([{"size": [4, 5], "counts": [5, 2, 2, 2, 2, 2, 4]}], "cuda:0")
    with pytest.raises(ValueError, match="sum"):
        rle.decode([{"size": [4, 6], "counts": good}], "cuda:0")
    with pytest.raises(ValueError, match="truncated"):
        rle.decode([{"size": [4, 5], "counts": good[:-1] + chr(ord(good[-1]) + 0x20)}], "cuda:0")
    with pytest.raises(ValueError, match="truncated"):
        rle.decode([{"size": [1030, 1030], "counts": "TQ\\P"}], "cuda:0")                   # the five-character count cut after four
    with pytest.raises(ValueError, match="sizes"):
        rle.decode([{"size": [4, 5], "counts": good}, {"size": [5, 4], "counts": good}], "cuda:0")
    with pytest.raises(ValueError):
        rle.decode([{"size": [4, 5], "counts": good[:-1] + "~"}], "cuda:0")                  # not a character of the format


def test_detections_entry_layout_and_bbox_rounding():
    """eval.py's collector on hand-made host inputs, the encoder stubbed: YOLACT's entry layout, [x, y, w, h] with the subtraction before the
    rounding to one decimal, category through the label map (class + 1 where the map has no such key), nothing for an empty frame."""
    import torch
    import eval as ev
    calls = []

    def stub(masks):
        calls.append(tuple(masks.shape))
        return [{"size": [int(masks.shape[1]), int(masks.shape[2])], "counts": "stub%d" % i} for i in range(masks.shape[0])]
    det = ev.Detections(encode=stub)
    boxes = torch.tensor([[10.04, 20.06, 110.26, 220.449], [0.0, 0.0, 639.0, 479.0], [3.25, 4.75, 3.25, 4.75]], dtype=torch.float32)
    result = {"pred_masks": torch.zeros(3, 6, 8, dtype=torch.bool), "pred_boxes": boxes, "pred_classes": torch.tensor([0, 0, 4]),
              "pred_scores": torch.tensor([0.9, 0.5, 0.25]), "pred_depth": None}
    det.add_frame(17, result, {1: 7})
    det.add_frame(18, {"pred_masks": None, "pred_boxes": None, "pred_classes": None, "pred_scores": None}, {1: 7})
    det.add_frame(19, dict(result, pred_masks=torch.zeros(0, 6, 8, dtype=torch.bool)), {1: 7})
    assert calls == [(3, 6, 8)] and len(det.bbox_data) == len(det.mask_data) == 3
    want = []
    for row in boxes.tolist():
        x0, y0, x1, y1 = row
        want.append([round(float(v) * 10) / 10 for v in (x0, y0, x1 - x0, y1 - y0)])
    assert want[0] == [10.0, 20.1, 100.2, 200.4] and want[2] == [3.2, 4.8, 0.0, 0.0]          # (round() on the float32 values: half to even)
    for i, (b, m) in enumerate(zip(det.bbox_data, det.mask_data)):
        assert list(b) == ["image_id", "category_id", "bbox", "score"] and list(m) == ["image_id", "category_id", "segmentation", "score"]
        assert b["image_id"] == m["image_id"] == 17 and b["category_id"] == m["category_id"] == (7 if i < 2 else 5)
        assert b["bbox"] == want[i] and m["segmentation"] == {"size": [6, 8], "counts": "stub%d" % i}
        assert b["score"] == m["score"] == float(result["pred_scores"][i]) and type(b["score"]) is float
    again = json.loads(json.dumps([det.bbox_data, det.mask_data]))
    assert again == [det.bbox_data, det.mask_data]


def test_detections_dump_writes_both_lists(tmp_path):
    import eval as ev
    det = ev.Detections(encode=lambda m: [])
    det.bbox_data.append({"image_id": 1, "category_id": 1, "bbox": [0.0, 1.0, 2.0, 3.0], "score": 0.5})
    det.mask_data.append({"image_id": 1, "category_id": 1, "segmentation": {"size": [3, 4], "counts": "228"}, "score": 0.5})
    bbox, mask = os.path.join(tmp_path, "a", "b", "bbox.json"), os.path.join(tmp_path, "c", "mask.json")
    det.dump(bbox, mask)
    with open(bbox) as f:
        assert json.load(f) == det.bbox_data
    with open(mask) as f:
        assert json.load(f) == det.mask_data
