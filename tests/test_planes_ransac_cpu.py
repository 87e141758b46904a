"""CPU: the robust plane fit's restatement (tests/planes_ransac_restate.py) -- Philox4x32-10 known answers, the recovery the feature is for,
the condition the device fuzz relies on (no undecided test in its inputs) -- and the host-side validation of prn_planes_ransac_*,
planes.fit_planes_ransac and the --plane_* flags of simple_inference.py."""
import ctypes

import numpy as np
import pytest
import torch

from planes_ransac_restate import DOMINANT, FUZZ, angle_deg, fuzz_reference, philox4x32_10, restate_ransac, two_plane_scene
from planes_restate import restate


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds"""
    assert tuple(int(w[0]) for w in philox4x32_10(counter, key)) == want


@pytest.mark.parametrize("H,W", [(37, 53), (60, 80)])
def test_restatement_recovers_the_dominant_plane_where_least_squares_does_not(H, W):
    """a mask with a quarter of its pixels on a second plane: 64 hypotheses + refit within 0.5 degrees of the dominant plane (4 x the worst
    case measured when the contract was written), the least-squares normal more than 10 degrees off (smallest measured: 35)"""
    for seed in range(20):
        depth, mask, K, _ = two_plane_scene(H, W, 0.25, seed)
        r = restate_ransac(depth, mask, K, threshold=0.03, hypotheses=64, seed=seed)
        assert bool(r["valid"][0]) and 0 <= int(r["hypothesis"][0]) < 64
        robust = angle_deg(r["planes"][0, :3], DOMINANT[0])
        _, lsq, ok = restate(depth, mask, K)
        plain = angle_deg(lsq[0, :3].numpy(), DOMINANT[0])
        print(H, W, seed, "robust %.4f deg, least squares %.2f deg, inliers %d of %d" % (robust, plain, int(r["inliers"][0]), int(r["count"][0])))
        assert bool(ok[0]) and robust <= 0.5 and plain > 10.0, (seed, robust, plain)


@pytest.mark.parametrize("cfg", FUZZ, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_fuzz_inputs_have_no_undecided_test(cfg):
    """a condition on the INPUTS of the device fuzz (exact agreement needs it), not a tolerance: a failure asks for another seed"""
    depth, masks, K, ref = fuzz_reference(cfg)
    assert ref["undecided"] == 0
    assert np.array_equal(ref["count"], masks.reshape(len(masks), -1).sum(1))
    assert np.array_equal(ref["inliers"], ref["inlier_masks"].reshape(len(masks), -1).sum(1)) and not (ref["inlier_masks"] & ~masks).any()
    v = ref["valid"]
    assert (ref["hypothesis"][v] >= 0).all() and (ref["hypothesis"][~v] == -1).all() and (ref["inliers"][~v] == 0).all() and np.isnan(ref["planes"][~v]).all()
    if cfg[0] >= 7:
        assert not v[2:6].any() and bool(v[1])                     # empty, 1 px, 2 px, line: invalid; the full-image mask: valid


def test_ws_bytes_refuses_invalid_sizes_and_grows():
    from planerecnet_amd import _lib
    ws = _lib.lib.prn_planes_ransac_ws_bytes
    for args in ((0, 1, 8, 8, 16), (1, -1, 8, 8, 16), (1, 1, 0, 8, 16), (1, 1, 8, 0, 16), (1, 1, 8, 8, 0), (1, 1, 8, 8, -3), (1, 1, 8, 8, 4097),
                 (1, 1, 65536, 65536, 16)):
        assert ws(*args) == -1, args
    base = ws(1, 10, 60, 80, 64)
    assert base > 0 and base % 256 == 0
    assert ws(1, 20, 60, 80, 64) > base and ws(1, 10, 60, 80, 4096) > base and ws(1, 0, 60, 80, 64) > 0
    assert ws(1, 10, 60, 80, 64) - _lib.lib.prn_planes_ws_bytes(1, 10, 60, 80) >= 10 * 64 * (4 * 8 + 4)       # hypotheses and scores


def test_entry_point_validates_before_any_launch():
    from planerecnet_amd import _lib
    lib = _lib.lib
    err = lambda: lib.prn_last_error().decode()      # noqa: E731
    p = ctypes.c_void_p(4096)                                       # (never dereferenced: validation precedes the launch)

    def call(threshold=0.05, relative=0, hypotheses=64, refine=1, B=1, Ntot=1, bufs=None, ws=None):
        b = [None] * 11 if bufs is None else bufs
        return lib.prn_planes_ransac_fit(b[0], b[1], b[2], b[3], B, Ntot, 8, 8, threshold, relative, hypotheses, refine, 5, b[4], b[5], b[6], b[7], b[8], b[9],
                                         b[10], ws, None)
    assert call(refine=-1) != 0 and "refine" in err()
    assert call(refine=9) != 0 and "refine" in err()
    assert call(hypotheses=0) != 0 and "hypotheses" in err()
    assert call(hypotheses=4097) != 0 and "hypotheses" in err()
    for t in (0.0, -0.1, float("inf"), float("nan")):
        assert call(threshold=t) != 0 and "threshold" in err(), t
    assert call(B=0) != 0 and "bad sizes" in err()
    assert call() != 0 and "null" in err()
    full = [p] * 11
    assert call(bufs=full[:4] + [None] + full[5:], ws=p) != 0 and "null output" in err()
    assert call(bufs=full, ws=ctypes.c_void_p(4100)) != 0 and "aligned" in err()


def test_api_refuses_bad_parameters_and_host_tensors():
    from planerecnet_amd import planes
    depth, masks, K = torch.zeros(1, 1, 8, 8), [torch.zeros(1, 8, 8, dtype=torch.bool)], torch.eye(3)
    for kw in ({"refine": -1}, {"refine": 9}, {"hypotheses": 0}, {"hypotheses": 4097}, {"hypotheses": 2.5}, {"threshold": 0.0}, {"threshold": -1.0},
               {"threshold": float("nan")}, {"threshold": float("inf")}, {"seed": -1}):
        with pytest.raises(ValueError):
            planes.fit_planes_ransac(depth, masks, K, **kw)
        with pytest.raises(ValueError):
            planes.planar_depth([{"pred_depth": depth, "pred_masks": masks[0]}], K, robust=kw)
    with pytest.raises(RuntimeError, match="device tensor"):
        planes.fit_planes_ransac(depth, masks, K)
    with pytest.raises(RuntimeError, match="device tensor"):
        planes.planar_depth([{"pred_depth": depth, "pred_masks": masks[0]}], K, robust={})


def test_command_line_maps_to_the_robust_options():
    import simple_inference as si
    si.parse_args([])
    assert si.robust_options() is None
    si.parse_args(["--plane_fit", "lsq", "--plane_threshold", "0.2"])
    assert si.robust_options() is None
    si.parse_args(["--plane_fit", "ransac"])
    assert si.robust_options() == {"threshold": 0.05, "relative": False, "hypotheses": 256, "refine": 1, "seed": 0}
    si.parse_args(["--plane_fit", "ransac", "--plane_threshold", "0.02", "--plane_relative", "--plane_hypotheses", "100", "--plane_refine", "2",
                   "--plane_seed", "7"])
    opts = si.robust_options()
    assert opts == {"threshold": 0.02, "relative": True, "hypotheses": 100, "refine": 2, "seed": 7}
    from planerecnet_amd import planes
    assert planes._robust_options(**opts) == opts                   # the keywords are fit_planes_ransac's
    for bad in (["--plane_hypotheses", "0"], ["--plane_refine", "9"], ["--plane_threshold", "-1"], ["--plane_fit", "median"]):
        with pytest.raises(SystemExit):
            si.parse_args(bad)
    si.parse_args([])
