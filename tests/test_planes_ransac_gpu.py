"""GPU: the robust plane fit on the device (csrc/prn_planes_ransac.hip through planes.fit_planes_ransac and planar_depth(robust=...)) against
the fp64 restatement (tests/planes_ransac_restate.py) -- exact in the chosen hypothesis and the inlier sets on the fuzzed ragged inputs --,
recovery of a dominant plane, exact planes, determinism and batching, no host synchronisation, and the planar depth painted from it."""
import numpy as np
import pytest
import torch

from planes_ransac_restate import DOMINANT, FUZZ, FUZZ_SEED, FUZZ_THRESHOLD, angle_deg, fuzz_reference, restate_ransac, two_plane_scene
from planes_restate import k_of, plane_depth_map
from test_planes_gpu import _fuzz_image

pytestmark = pytest.mark.gpu


def _planes():
    from planerecnet_amd import planes
    return planes


def _dev(depth, masks):
    return torch.from_numpy(depth)[None, None].cuda(), torch.from_numpy(masks).cuda()


def _same(a, b):
    """bit-identical up to the payload of NaNs"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.is_floating_point():
        return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(123.0), b.nan_to_num(123.0))
    return torch.equal(a, b)


def _check_against_restatement(got, ref, masks):
    """got: the six per-image tensors of one image; ref: restate_ransac's dict"""
    planes, valid, count, inliers, hypothesis, inlier_masks = [t.cpu() for t in got]
    v = torch.from_numpy(ref["valid"])
    assert torch.equal(valid, v), (valid.tolist(), v.tolist())
    assert torch.equal(count, torch.from_numpy(masks.reshape(len(masks), -1).sum(1)))
    assert inlier_masks.dtype == torch.bool and inlier_masks.shape == masks.shape
    assert torch.equal(hypothesis[v], torch.from_numpy(ref["hypothesis"])[v])
    assert torch.equal(inliers[v], torch.from_numpy(ref["inliers"])[v])
    assert torch.equal(inlier_masks[v], torch.from_numpy(ref["inlier_masks"])[v])
    assert torch.isnan(planes[~v]).all() and not inliers[~v].any() and bool((hypothesis[~v] == -1).all()) and not inlier_masks[~v].any()
    if v.any():
        rp = torch.from_numpy(ref["planes"])
        assert float((planes[v, :3] * rp[v, :3]).sum(1).min()) >= 1 - 1e-12
        assert float(((planes[v, 3] - rp[v, 3]).abs() / rp[v, 3].abs().clamp_min(1e-6)).max()) <= 1e-9


@pytest.mark.parametrize("cfg", FUZZ, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_fuzz_agrees_exactly_with_the_restatement(cfg):
    N, H, W, hypotheses, relative, refine = cfg
    depth, masks, K, ref = fuzz_reference(cfg)
    assert ref["undecided"] == 0                                    # (the condition under which exact agreement is owed)
    d, m = _dev(depth, masks)
    got = _planes().fit_planes_ransac(d, [m], K, threshold=FUZZ_THRESHOLD, relative=relative, hypotheses=hypotheses, refine=refine, seed=FUZZ_SEED)
    _check_against_restatement([t[0] for t in got], ref, masks)
    if N >= 7:
        assert not got[1][0][2:6].any() and bool(got[1][0][1])       # empty, 1 px, 2 px, line: invalid; the full-image mask: valid


@pytest.mark.parametrize("H,W", [(37, 53), (60, 80)])
def test_dominant_plane_is_recovered(H, W):
    depth, mask, K, region = two_plane_scene(H, W, 0.25, seed=3)
    d, m = _dev(depth, mask)
    planes, valid, count, inliers, hypothesis, inlier_masks = _planes().fit_planes_ransac(d, [m], K, threshold=0.03, hypotheses=64, seed=3)
    lsq, lsq_valid, _ = _planes().fit_planes(d, [m], K)
    assert bool(valid[0][0]) and bool(lsq_valid[0][0]) and int(count[0][0]) == int(mask.sum())
    robust, plain = angle_deg(planes[0][0, :3].cpu().numpy(), DOMINANT[0]), angle_deg(lsq[0][0, :3].cpu().numpy(), DOMINANT[0])
    print(H, W, "robust %.4f deg, least squares %.2f deg" % (robust, plain))
    assert robust <= 0.5 and plain > 10.0, (robust, plain)
    inl = inlier_masks[0][0].cpu().numpy()
    assert int(inliers[0][0]) == int(inl.sum()) and not (inl & ~mask[0]).any()
    assert (inl & region).sum() > 0.9 * inl.sum()


def test_exact_planes_stay_exact():
    """the noise-free planes of test_planes_gpu.test_exact_planes_are_recovered: the robust fit returns the least-squares normal (1e-5 rad),
    every mask pixel an inlier"""
    H, W = 96, 128
    K = k_of(110.0, 100.0, 63.5, 47.5)
    truth = [([0.0, 0.0, 1.0], 3.0), ([0.3, -0.5, 1.0], 2.0), ([-1.0, 0.2, 0.6], 1.2), ([0.0, 1.0, 0.1], 1.4), ([0.2, 0.1, 1.0], 4.0), ([0.1, 0.1, -1.0], -2.5)]
    boxes = [(0, 96, 0, 128), (10, 60, 20, 90), (30, 90, 0, 40), (50, 96, 0, 128), (5, 40, 60, 128), (20, 70, 30, 100)]
    for (n, off), (y0, y1, x0, x1) in zip(truth, boxes):
        n = np.asarray(n) / np.linalg.norm(n)
        pd = plane_depth_map(n, off, K, H, W)
        m = np.zeros((1, H, W), bool)
        m[0, y0:y1, x0:x1] = True
        m[0] &= pd > 0
        d, mt = _dev(pd.astype(np.float32), m)
        lsq, lsq_valid, _ = _planes().fit_planes(d, [mt], K)
        planes, valid, count, inliers, _, inlier_masks = _planes().fit_planes_ransac(d, [mt], K, threshold=0.01, hypotheses=32, refine=1, seed=1)
        assert bool(valid[0][0]) and bool(lsq_valid[0][0])
        ang = float(torch.arccos((planes[0][0, :3] * lsq[0][0, :3]).sum().clamp(max=1.0)))
        assert ang <= 1e-5, (n, ang)
        assert int(inliers[0][0]) == int(count[0][0]) == int(m.sum()) and torch.equal(inlier_masks[0], mt)


@pytest.fixture(scope="module")
def ragged():
    H, W = 60, 80
    rng = np.random.RandomState(7)
    Ks = [k_of(80.0, 82.0, 39.5, 29.5), k_of(75.0, 70.0, 41.0, 28.0), k_of(90.0, 90.0, 40.0, 30.0)]
    imgs = [_fuzz_image(rng, n, H, W, k) for n, k in zip((0, 3, 100), Ks)]
    return Ks, imgs


def test_ragged_batch_is_bit_identical_to_per_image_calls_and_repeats(ragged):
    Ks, imgs = ragged
    depth = torch.cat([torch.from_numpy(d)[None, None] for d, _ in imgs]).cuda()
    masks = [None] + [torch.from_numpy(m).cuda() for _, m in imgs[1:]]
    kb = torch.from_numpy(np.stack(Ks))
    kw = {"threshold": 0.02, "hypotheses": 100, "refine": 1}
    batched = _planes().fit_planes_ransac(depth, masks, kb, seed=5, **kw)
    assert batched[0][0].shape == (0, 4) and batched[5][0].shape == (0, 60, 80) and batched[5][0].dtype == torch.uint8
    for b in range(3):
        one = _planes().fit_planes_ransac(depth[b:b + 1], [masks[b]], Ks[b], seed=5, **kw)
        for got, want in zip(one, batched):
            assert _same(got[0], want[b]), b
    for _ in range(10):
        again = _planes().fit_planes_ransac(depth, masks, kb, seed=5, **kw)
        for got, want in zip(again, batched):
            for b in range(3):
                assert _same(got[b], want[b])
    other = _planes().fit_planes_ransac(depth, masks, kb, seed=6, **kw)
    assert not torch.equal(torch.cat(other[4]), torch.cat(batched[4]))                    # another seed: other draws
    for seed, res in ((5, batched), (6, other)):
        for b in (1, 2):
            ref = restate_ransac(imgs[b][0], imgs[b][1], Ks[b], seed=seed, **kw)
            assert ref["undecided"] == 0
            _check_against_restatement([t[b] for t in res], ref, imgs[b][1])
    assert torch.equal(torch.cat(other[2]), torch.cat(batched[2]))


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
        out = _planes().planar_depth(results, K, depth_range=(0.0, 10.0), robust={"threshold": 0.02, "hypotheses": 64})
        fit = _planes().fit_planes_ransac(results[0]["pred_depth"], [results[0]["pred_masks"]], k_dev, threshold=0.02, hypotheses=64)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert set(results[0]) == set(keep)
    for k, v in keep.items():
        assert torch.equal(results[0][k], v), k
    assert out[0] is not results[0] and _same(out[0]["pred_planes"], fit[0][0]) and torch.equal(out[0]["pred_plane_inlier_masks"], fit[5][0])


def test_planar_depth_with_the_robust_fit(ragged):
    Ks, imgs = ragged
    results = [{"pred_depth": torch.from_numpy(d)[None, None].cuda(), "pred_masks": torch.from_numpy(m).cuda()} for d, m in imgs]
    results[0]["pred_masks"] = None
    kb = torch.from_numpy(np.stack(Ks))
    opts = {"threshold": 0.02, "hypotheses": 100, "seed": 5}
    plain = _planes().planar_depth(results, kb, depth_range=(0.5, 8.0))
    same = _planes().planar_depth(results, kb, depth_range=(0.5, 8.0), robust=None)
    robust = _planes().planar_depth(results, kb, depth_range=(0.5, 8.0), robust=opts)
    unranged = [_planes().planar_depth(results, kb, robust=o) for o in (None, opts)]          # (no NaN rule: a painted pixel shows its plane)
    fit =_planes().fit_planes_ransac(torch.cat([r["pred_depth"] for r in results]), [r["pred_masks"] for r in results], kb, **opts)
    for b in range(3):
        assert set(same[b]) == set(plain[b]) and "pred_plane_inliers" not in plain[b]
        for key in ("pred_planes", "pred_plane_valid", "pred_plane_depth"):
            assert _same(same[b][key], plain[b][key]), (b, key)
        assert _same(robust[b]["pred_planes"], fit[0][b]) and torch.equal(robust[b]["pred_plane_valid"], fit[1][b])
        assert torch.equal(robust[b]["pred_plane_inliers"], fit[3][b]) and torch.equal(robust[b]["pred_plane_inlier_masks"], fit[5][b])
        assert "pred_plane_masks" not in robust[b]
        # the same instances are valid, so the same pixels are painted: in both runs every pixel a valid instance covers shows the plane of the
        # highest-index valid covering instance (fp32 of the fp64 plane depth: 1e-6 as in test_planes_gpu), every other pixel the prediction
        assert torch.equal(robust[b]["pred_plane_valid"], plain[b]["pred_plane_valid"]), b
        pred = imgs[b][0]
        for run in unranged:
            want, owned = pred.astype(np.float64), np.zeros(pred.shape, bool)
            if results[b]["pred_masks"] is not None:
                for i in np.flatnonzero(run[b]["pred_plane_valid"].cpu().numpy()):
                    p = run[b]["pred_planes"][i].cpu().numpy()
                    want = np.where(imgs[b][1][i], plane_depth_map(p[:3], p[3], Ks[b], 60, 80), want)
                    owned |= imgs[b][1][i]
            got = run[b]["pred_plane_depth"].squeeze().cpu().numpy()
            assert np.array_equal(got[~owned], pred[~owned])
            assert np.abs(got[owned] / want[owned] - 1.0).max(initial=0.0) <= 1e-6
    assert robust[0]["pred_plane_inlier_masks"].shape == (0, 60, 80)
    assert any(not _same(robust[b]["pred_planes"], plain[b]["pred_planes"]) for b in (1, 2))


def test_ibims1_planar_depth_exporter_takes_the_plane_fit_flags(tmp_path):
    """simple_inference.py --ibims1_pd with --plane_fit ransac writes the robust planar depth; without the flag, the least-squares one as before
    (the exporter in process, a stand-in for the network that returns the two-plane scene)"""
    sio = pytest.importorskip("scipy.io")
    import simple_inference as si
    from planerecnet_amd.config import cfg, set_cfg
    set_cfg("PlaneRecNet_50_config")                               # (the input staging reads the backbone's transform)
    H, W = 60, 80
    depth, mask, K, _ = two_plane_scene(H, W, 0.25, seed=2)
    result = {"pred_depth": torch.from_numpy(depth)[None, None].cuda(), "pred_masks": torch.from_numpy(mask).cuda()}
    (tmp_path / "in").mkdir()
    sio.savemat(str(tmp_path / "in" / "scene.mat"), {"data": {"rgb": np.zeros((H, W, 3), np.uint8), "calib": K.T}})
    flags = ["--plane_fit", "ransac", "--plane_threshold", "0.03", "--plane_hypotheses", "64", "--plane_seed", "2"]
    old_device = cfg.device
    cfg.device = "cuda:0"
    try:
        for name, argv in (("ransac", flags), ("lsq", [])):
            si.parse_args(argv)
            si.ibims1_pd(lambda batch: [dict(result)], str(tmp_path / "in"), str(tmp_path / name))
    finally:
        cfg.device = old_device
        si.parse_args([])
    got = {}
    for name, robust in (("ransac", {"threshold": 0.03, "hypotheses": 64, "seed": 2}), ("lsq", None)):
        assert (tmp_path / name / "scene_results.png").exists()
        got[name] = sio.loadmat(str(tmp_path / name / "scene_results.mat"))["pred_depths"]
        want = _planes().planar_depth([result], K, depth_range=(0.0, 10.0), robust=robust)[0]["pred_plane_depth"].squeeze().cpu().numpy()
        assert got[name].dtype == np.float32 and np.array_equal(got[name], want, equal_nan=True)
    assert not np.array_equal(got["ransac"], got["lsq"], equal_nan=True)


@pytest.mark.parametrize("clean", [None, {"keep": "largest"}])
def test_planar_depth_paints_the_dominant_plane(clean):
    H, W = 60, 80
    depth, mask, K, region = two_plane_scene(H, W, 0.25, seed=4)
    truth = plane_depth_map(DOMINANT[0], DOMINANT[1], K, H, W)
    res = [{"pred_depth": torch.from_numpy(depth)[None, None].cuda(), "pred_masks": torch.from_numpy(mask).cuda()}]
    plain = _planes().planar_depth(res, K, clean=clean)[0]
    robust = _planes().planar_depth(res, K, clean=clean, robust={"threshold": 0.03, "hypotheses": 64, "seed": 4})[0]
    assert ("pred_plane_masks" in robust) == (clean is not None)
    used = robust["pred_plane_masks"] if clean is not None else res[0]["pred_masks"]
    if clean is not None:
        assert torch.equal(used, plain["pred_plane_masks"])
        fit = _planes().fit_planes_ransac(res[0]["pred_depth"], [used], K, threshold=0.03, hypotheses=64, seed=4)
        assert _same(robust["pred_planes"], fit[0][0]) and torch.equal(robust["pred_plane_inlier_masks"], fit[5][0])
    sel = used[0].cpu().numpy() & region
    err = lambda r: np.abs(r["pred_plane_depth"].squeeze().cpu().numpy().astype(np.float64)[sel] / truth[sel] - 1.0).max()      # noqa: E731
    assert bool(robust["pred_plane_valid"][0]) and bool(plain["pred_plane_valid"][0])
    print("painted depth of the dominant region: robust %.4f, least squares %.3f (relative)" % (err(robust), err(plain)))
    assert err(robust) <= 0.01 < err(plain)
