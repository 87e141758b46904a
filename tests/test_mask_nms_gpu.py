"""GPU: greedy mask NMS on the device (planerecnet_amd/nms.py: mask_nms / mask_nms_batched, csrc/prn_mask_nms.hip) against the keep vectors
of the real reference (tests/golden/mask_nms.npz) and the numpy restatements (tests/mask_nms_restate.py): candidate counts at the edges of
the 64-bit suppression words, mask sizes at the edges of the 32-bit packed words, a ragged batch, no host synchronisation, untouched
inputs, and PlaneRecNet.inference in mask mode.  Every comparison is exact (torch.equal)."""
import os

import numpy as np
import pytest
import torch

import mask_nms_restate as R

pytestmark = pytest.mark.gpu

CN = "PlaneRecNet_50_config"


def _nms():
    from planerecnet_amd import nms
    return nms


def _dev(labels, masks, sums, dtype=torch.bool):
    return torch.from_numpy(labels).cuda(), torch.from_numpy(masks).to(dtype).cuda(), torch.from_numpy(sums).cuda()


def _expect(keep_u8, dtype=torch.bool):
    return torch.from_numpy(np.asarray(keep_u8, np.uint8)).to(dtype)


def test_fixture_cases_through_mask_nms(golden_dir):
    fixture = np.load(os.path.join(golden_dir, "mask_nms.npz"))
    for name, (labels, masks, sums, thr) in R.cases().items():
        for dtype in (torch.bool, torch.uint8):
            l, m, s = _dev(labels, masks, sums, dtype)
            keep = _nms().mask_nms(l, m, s, torch.linspace(0.9, 0.1, len(labels)).cuda(), nms_thr=thr)
            assert keep.is_cuda and keep.dtype == dtype and keep.shape == (len(labels),)
            assert torch.equal(keep.cpu(), _expect(fixture["keep_" + name], dtype)), name


N_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 500)
SHAPES = ((1, 1), (1, 31), (1, 32), (1, 33), (5, 7), (37, 65), (120, 160))
WORD_EDGE_CASES = [(n, h, w) for (h, w) in SHAPES for n in (N_EDGES if (h, w) == (37, 65) else (65, 129))]


@pytest.mark.parametrize("n,h,w", WORD_EDGE_CASES, ids=["n%d-%dx%d" % c for c in WORD_EDGE_CASES])
def test_candidate_counts_and_mask_sizes_at_the_word_edges(n, h, w):
    """n round the 64-candidate words of the suppression matrix / removed set, H*W round the 32-pixel words of the packed masks (most mask
    base addresses are then not 16-byte aligned)."""
    labels, masks, sums, _ = R.clustered(1000 + 7 * n + h * w, n, h, w, n_labels=1 + n % 2)
    thr = (0.3, 0.5, 0.1)[n % 3]
    want = R.row_vectorised(labels, masks, sums, thr)
    if n <= 129:
        assert np.array_equal(R.reference_loop(labels, masks, sums, thr), want)
    keep = _nms().mask_nms(*_dev(labels, masks, sums), torch.zeros(n).cuda(), nms_thr=thr)
    assert torch.equal(keep.cpu(), _expect(want))
    if h * w >= 35 and n >= 63:
        assert 0 < int(want.sum()) < n                                                  # (something falls, something stays)


def test_three_labels():
    labels, masks, sums, _ = R.clustered(77, 130, 37, 65, n_labels=3)
    assert len(set(labels.tolist())) == 3
    want = R.reference_loop(labels, masks, sums, 0.3)
    assert not np.array_equal(want, R.reference_loop(np.zeros_like(labels), masks, sums, 0.3))      # (the labels matter in this case)
    keep = _nms().mask_nms(*_dev(labels, masks, sums), torch.zeros(130).cuda(), nms_thr=0.3)
    assert torch.equal(keep.cpu(), _expect(want))


def test_the_limit_of_4096_candidates():
    """One wave holds the removed set of an image: 64 lanes x 64 bits.  All 64 blocks of 64 candidates, against the row-vectorised restatement."""
    n = _nms().MASK_NMS_MAX
    assert n == 4096
    labels, masks, sums, _ = R.clustered(4096, n, 8, 8, n_labels=2, drop=0.2)
    want = R.row_vectorised(labels, masks, sums, 0.5)
    assert 0.02 * n < int(want.sum()) < 0.98 * n and int(want[n // 2:].sum()) > 0       # survivors in the late blocks too
    keep = _nms().mask_nms(*_dev(labels, masks, sums), torch.zeros(n).cuda(), nms_thr=0.5)
    assert torch.equal(keep.cpu(), _expect(want))
    l1, m1, s1 = torch.zeros(n + 1, dtype=torch.long).cuda(), torch.ones(n + 1, 1, 1, dtype=torch.bool).cuda(), torch.ones(n + 1).cuda()
    with pytest.raises(RuntimeError, match="limit"):
        _nms().mask_nms_batched(l1, m1, s1, [n + 1])
    both = _nms().mask_nms_batched(l1, m1, s1, [n, 1])                                  # ... which is per image
    assert int(both.sum()) == 2 and bool(both[0]) and bool(both[n])


def _ragged():
    counts = [65, 0, 1, 130, 64]
    h, w = 20, 28                                                                       # 560 pixels: 17.5 words, mask bases 16-byte aligned or not
    parts = [R.clustered(300 + b, c, h, w, n_labels=2) for b, c in enumerate(counts)]
    for b in (3, 4):                                                                    # the best mask of image 0 again, as the best of images 3 and 4
        parts[b][0][0], parts[b][1][0], parts[b][2][0] = parts[0][0][0], parts[0][1][0], parts[0][2][0]
    labels, masks, sums = (np.concatenate([p[k] for p in parts]) for k in range(3))
    return counts, parts, labels, masks, sums


def test_ragged_batch_equals_per_segment_calls_and_the_restatement():
    counts, parts, labels, masks, sums = _ragged()
    thr = 0.3
    l, m, s = _dev(labels, masks, sums)
    keep = _nms().mask_nms_batched(l, m, s, counts, nms_thr=thr)
    assert keep.shape == (sum(counts),) and keep.dtype == torch.bool
    want = np.concatenate([R.reference_loop(p[0], p[1], p[2], thr) for p in parts])
    assert torch.equal(keep.cpu(), _expect(want))
    o = 0
    for c in counts:
        one = _nms().mask_nms(l[o:o + c], m[o:o + c], s[o:o + c], torch.zeros(c).cuda(), nms_thr=thr)
        if c == 0:
            assert one == []
        else:
            assert torch.equal(one, keep[o:o + c])
        o += c
    # an image's best candidate always stays -- the planted copies too: segments do not see each other.  In ONE segment the copies fall
    assert all(bool(keep[o]) for o in (0, 66, 196))
    merged = R.reference_loop(labels, masks, sums, thr)
    assert merged[0] == 1 and merged[66] == 0 and merged[196] == 0
    assert torch.equal(_nms().mask_nms_batched(l, m, s, [sum(counts)], nms_thr=thr).cpu(), _expect(merged))


def test_no_host_synchronisation():
    """Fails on a host implementation: that one downloads the suppression matrix."""
    counts, _, labels, masks, sums = _ragged()
    l, m, s = _dev(labels, masks, sums)
    scores = torch.zeros(counts[0]).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda").item()                                         # the mode does catch a synchronisation
        batched = _nms().mask_nms_batched(l, m, s, counts, nms_thr=0.3)
        single = _nms().mask_nms(l[:counts[0]], m[:counts[0]], s[:counts[0]], scores, nms_thr=0.3)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.equal(batched[:counts[0]], single) and 0 < int(single.sum()) < counts[0]


def test_inputs_are_untouched_any_mask_dtype_and_two_runs_agree():
    counts, _, labels, masks, sums = _ragged()
    want = _expect(np.concatenate([R.row_vectorised(labels[o:o + c], masks[o:o + c], sums[o:o + c], 0.5)
                                   for o, c in zip(np.cumsum([0] + counts[:-1]), counts)]), torch.uint8)
    rng = np.random.RandomState(3)
    weights = torch.from_numpy(rng.randint(1, 256, masks.shape).astype(np.uint8))
    variants = {"bool": torch.from_numpy(masks), "uint8": torch.from_numpy(masks).to(torch.uint8) * weights,      # non-zero = set
                "float32": torch.from_numpy(masks).float() * 0.25, "int64": torch.from_numpy(masks).long() * -3}
    for name, mk in variants.items():
        l, m, s = torch.from_numpy(labels).int().cuda(), mk.cuda(), torch.from_numpy(sums).double().cuda()      # labels -> .long(), sums -> .float()
        before = (l.clone(), m.clone(), s.clone())
        first = _nms().mask_nms_batched(l, m, s, counts, nms_thr=0.5)
        again = _nms().mask_nms_batched(l, m, s, counts, nms_thr=0.5)
        assert first.dtype == m.dtype and torch.equal(first, again), name
        assert torch.equal((first != 0).cpu().to(torch.uint8), want), name
        for a, b in zip((l, m, s), before):
            assert torch.equal(a, b), name
    # a non-contiguous view of the masks is read as what it shows
    wide = torch.zeros(masks.shape[0], masks.shape[1], masks.shape[2] + 3, dtype=torch.bool).cuda()
    wide[:, :, 3:] = torch.from_numpy(masks).cuda()
    view = wide[:, :, 3:]
    assert not view.is_contiguous()
    keep = _nms().mask_nms_batched(torch.from_numpy(labels).cuda(), view, torch.from_numpy(sums).cuda(), counts, nms_thr=0.5)
    assert torch.equal(keep.cpu().to(torch.uint8), want)


def test_empty_and_mismatched_calls():
    nms = _nms()
    none = nms.mask_nms_batched(torch.zeros(0, dtype=torch.long).cuda(), torch.zeros(0, 4, 4, dtype=torch.bool).cuda(), torch.zeros(0).cuda(), [0, 0])
    assert none.shape == (0,) and none.dtype == torch.bool and none.is_cuda
    assert nms.mask_nms(torch.zeros(0, dtype=torch.long).cuda(), torch.zeros(0, 4, 4, dtype=torch.bool).cuda(), torch.zeros(0).cuda(), torch.zeros(0).cuda()) == []
    l, m, s = torch.zeros(5, dtype=torch.long).cuda(), torch.ones(5, 4, 4, dtype=torch.bool).cuda(), torch.full((5,), 16.0).cuda()
    for counts in ([4], [3, 3], [], [6, -1]):
        with pytest.raises(RuntimeError, match="counts"):
            nms.mask_nms_batched(l, m, s, counts)
    with pytest.raises(RuntimeError, match="device tensors"):
        nms.mask_nms_batched(l.cpu(), m, s, [5])
    assert nms.mask_nms_batched(l, m, s, [2, 0, 3]).tolist() == [True, False, True, False, False]


@pytest.fixture(scope="module")
def net():
    from oracle import synth
    from planerecnet_amd.config import cfg, set_cfg
    from planerecnet_amd.planerecnet import PlaneRecNet
    set_cfg(CN)
    net = PlaneRecNet(cfg)
    net.load_state_dict(synth.make_state_dict(CN, seed=1))
    net = net.cuda()
    net.nms_type = "mask"
    return net


def _heads(net):
    """Synthetic head outputs shaped like test_model_gpu.py::test_batched_post_process_equals_image_by_image (B = 4 at 60x80; image 1 without a
    candidate, the candidates of image 2 all filtered out), with the dynamic kernels of an image drawn round three base kernels: candidates
    of one base predict nearly the same mask, so greedy NMS has something to remove."""
    g = torch.Generator().manual_seed(31)
    B, E, h, w = 4, net.inst_head.num_kernels, 60, 80
    C = net.inst_head.num_classes
    masks = torch.randn(B, E, h, w, generator=g) * 0.5
    masks[2] = 1.0
    depth = torch.rand(B, 1, 2 * h, 2 * w, generator=g) * 4 + 0.3
    base = torch.randn(B, 3, E, generator=g) * 0.3
    cates, kerns = [], []
    for S in net.num_grids:
        c = torch.where(torch.rand(B, S, S, C, generator=g) < 0.02, 0.3 + 0.6 * torch.rand(B, S, S, C, generator=g), torch.zeros(B, S, S, C))
        c[1] = 0.0
        cates.append(c.cuda())
        which = torch.randint(0, 3, (B, S, S), generator=g)
        k = torch.stack([base[b][which[b]] for b in range(B)]).permute(0, 3, 1, 2) + 0.02 * torch.randn(B, E, S, S, generator=g)
        k[2] = -3.0
        kerns.append(k.contiguous().cuda())
    return masks.cuda(), cates, kerns, depth.cuda(), [torch.empty(3, 4 * h, 4 * w) for _ in range(B)], (B, E, h, w, C)


def _same(ra, rb):
    for key in ("pred_masks", "pred_boxes", "pred_classes", "pred_scores", "pred_depth"):
        assert (ra[key] is None) == (rb[key] is None), key
        if ra[key] is not None:
            assert torch.equal(ra[key], rb[key]), key


def test_model_inference_in_mask_mode(net, monkeypatch):
    nms = _nms()
    masks, cates, kerns, depth, imgs, (B, E, h, w, C) = _heads(net)
    real, calls = nms.mask_nms_batched, []

    def counted(cate_labels, seg_masks, sum_masks, counts, nms_thr=0.5):
        calls.append(list(counts))
        return real(cate_labels, seg_masks, sum_masks, counts, nms_thr=nms_thr)

    seen = []

    def restated(cate_labels, seg_masks, sum_masks, counts, nms_thr=0.5):
        l, m, s = cate_labels.cpu().numpy(), seg_masks.cpu().numpy(), sum_masks.cpu().numpy()
        keep, o = [], 0
        for c in counts:
            keep.append(R.reference_loop(l[o:o + c], m[o:o + c], s[o:o + c], nms_thr))
            o += c
        seen.append(np.concatenate(keep))
        return torch.from_numpy(seen[-1]).to(seg_masks.dtype).to(seg_masks.device)

    with torch.no_grad():
        monkeypatch.setattr(nms, "mask_nms_batched", counted)
        batch = net.inference(masks, cates, kerns, depth, imgs)
        assert len(calls) == 1 and len(calls[0]) == 2 and min(calls[0]) > 1            # ONE call for the batch: the two images with candidates
        del calls[:]
        single = []
        for b in range(B):
            cate_b = torch.cat([c[b].reshape(-1, C) for c in cates], 0)
            kern_b = torch.cat([k[b].permute(1, 2, 0).reshape(-1, E) for k in kerns], 0)
            single.append(net.inference_single_image(masks[b:b + 1], cate_b, kern_b, depth[b:b + 1], (4 * h, 4 * w)))
        assert [len(c) for c in calls] == [1, 1]
        monkeypatch.setattr(nms, "mask_nms_batched", restated)
        oracle = net.inference(masks, cates, kerns, depth, imgs)
    assert batch[1]["pred_scores"] is None and batch[2]["pred_scores"] is None
    assert batch[0]["pred_scores"] is not None and batch[3]["pred_scores"] is not None
    assert len(seen) == 1 and 0 < int(seen[0].sum()) < len(seen[0])                     # the NMS removed some candidates and kept some
    for b in range(B):
        _same(batch[b], single[b])
        _same(batch[b], oracle[b])
    for b in (0, 3):
        assert not batch[b]["pred_boxes"].is_cuda and batch[b]["pred_masks"].shape[1:] == (4 * h, 4 * w)
        assert (batch[b]["pred_scores"][:-1] >= batch[b]["pred_scores"][1:]).all()
