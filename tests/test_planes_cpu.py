"""CPU: the plane fit / planar depth restatement (tests/planes_restate.py) against the reference's iBims-1 exporter (golden fixture),
the host-side validation of the prn_planes_* entry points, and the iBims-1 file conventions of simple_inference.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from planes_restate import k_of, plane_depth_map, restate

K0 = k_of(150.0, 145.0, 79.5, 59.5)


def test_restatement_reproduces_the_reference_exporter(golden_dir):
    z = np.load(os.path.join(golden_dir, "plane_depth.npz"))
    for b in range(z["depth"].shape[0]):
        ref = z["pred_depths"][b]
        got, planes, valid = restate(z["depth"][b], z["masks%d" % b], z["calib"][b].T, depth_range=(0.0, 10.0))
        assert bool(valid.all())
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).any()
        f = ~np.isnan(ref)
        assert np.max(np.abs(got[f].astype(np.float64) - ref[f]) / np.abs(ref[f])) <= 1e-12
        assert (planes[:, 3] >= 0).all() and torch.allclose(planes[:, :3].norm(dim=1), torch.ones(len(planes), dtype=torch.float64))


def test_restatement_recovers_exact_planes_and_rejects_degenerate_masks():
    H, W = 48, 64
    rng = np.random.RandomState(0)
    n = np.array([0.3, -0.4, 1.0])
    n /= np.linalg.norm(n)
    depth = plane_depth_map(n, 2.5, K0, H, W)
    masks = np.zeros((5, H, W), bool)
    masks[0, 10:40, 5:50] = rng.rand(30, 45) > 0.2
    masks[1, 3, 7] = True                                          # 1 pixel (the reference raises)
    masks[2, 3, 7:9] = True                                        # 2 pixels (the reference returns an arbitrary plane)
    masks[3, 20, :] = True                                         # a 1-pixel line on planar depth: collinear points
    # instance 4 stays empty
    out, planes, valid = restate(depth.astype(np.float32), masks, K0)
    assert valid.tolist() == [True, False, False, False, False]
    assert float(np.arccos(min(1.0, abs(float(planes[0, :3] @ torch.from_numpy(n)))))) <= 1e-5
    assert abs(float(planes[0, 3]) - 2.5) <= 2.5e-5
    assert torch.isnan(planes[1:]).all()
    # invalid instances take no part: their pixels keep the prediction (instance 3's line lies over instance 0: instance 0 wins there)
    assert out[3, 7] == np.float32(depth[3, 7]) and out[3, 8] == np.float32(depth[3, 8])
    line = masks[0, 20] & masks[3, 20]
    assert np.allclose(out[20][line], depth[20][line], rtol=1e-5)


def test_ws_bytes_refuses_invalid_sizes():
    from planerecnet_amd import _lib
    lib = _lib.lib
    assert lib.prn_planes_ws_bytes(1, 100, 480, 640) == 100 * 300 * 10 * 8 + 480 * 640 * 4
    assert lib.prn_planes_ws_bytes(2, 0, 120, 160) == (2 * 120 * 160 * 4 + 255) // 256 * 256 + 0
    for args in ((0, 1, 8, 8), (-1, 1, 8, 8), (1, -1, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0), (1, 1, 65536, 65536)):
        assert lib.prn_planes_ws_bytes(*args) == -1, args


def test_entry_points_validate_before_any_launch():
    from planerecnet_amd import _lib
    lib = _lib.lib
    err = lambda: lib.prn_last_error().decode()      # noqa: E731
    p = ctypes.c_void_p(4096)                                       # (never dereferenced: validation precedes the launch)
    assert lib.prn_planes_fit(p, p, p, p, 0, 1, 8, 8, p, p, p, p, p, None) != 0 and "bad sizes" in err()
    assert lib.prn_planes_fit(p, p, p, p, 1, -2, 8, 8, p, p, p, p, p, None) != 0 and "bad sizes" in err()
    assert lib.prn_planes_fit(p, None, p, p, 1, 1, 8, 8, p, p, p, p, p, None) != 0 and "null" in err()
    assert lib.prn_planes_fit(p, p, p, p, 1, 1, 8, 8, None, p, p, p, p, None) != 0 and "null output" in err()
    assert lib.prn_planes_fit(p, p, p, p, 1, 1, 8, 8, p, p, p, p, ctypes.c_void_p(4100), None) != 0 and "aligned" in err()
    assert lib.prn_planes_render(p, p, p, p, p, p, 1, 1, 8, 8, 0, 0.0, 0.0, p, p, None) != 0 and "alias" in err()
    assert lib.prn_planes_render(p, p, p, p, p, p, 1, 1, 8, 8, 1, 10.0, 0.0, ctypes.c_void_p(8192), p, None) != 0 and "range" in err()
    assert lib.prn_planes_render(p, p, p, p, None, p, 1, 1, 8, 8, 0, 0.0, 0.0, ctypes.c_void_p(8192), p, None) != 0 and "planes" in err()
    assert lib.prn_planes_render(p, p, p, p, p, p, 1, 1, 0, 8, 0, 0.0, 0.0, ctypes.c_void_p(8192), p, None) != 0 and "bad sizes" in err()


def test_planes_api_refuses_host_tensors():
    from planerecnet_amd import planes
    with pytest.raises(RuntimeError, match="device tensor"):
        planes.fit_planes(torch.zeros(1, 1, 8, 8), [torch.zeros(1, 8, 8, dtype=torch.bool)], torch.eye(3))


def test_ibims1_file_conventions(tmp_path):
    sio = pytest.importorskip("scipy.io")
    import simple_inference as si
    rng = np.random.RandomState(3)
    rgb = rng.randint(0, 256, size=(6, 8, 3)).astype(np.uint8)
    K = k_of(520.0, 515.0, 320.5, 240.25)
    os.makedirs(tmp_path / "in")
    for name in ("b_scene", "a_scene"):
        sio.savemat(str(tmp_path / "in" / (name + ".mat")), {"data": {"rgb": rgb, "calib": K.T}})
    (tmp_path / "in" / "notes.txt").write_text("not an input")
    got = si.ibims1_inputs(str(tmp_path / "in"))
    assert [n for n, _ in got] == ["a_scene", "b_scene"]
    r, k = si.read_ibims1_mat(got[0][1])
    assert r.dtype == np.uint8 and np.array_equal(r, rgb)
    assert k.dtype == np.float64 and np.array_equal(k, K)           # K = calib.T
    assert si.ibims1_outputs("out", "a_scene") == (os.path.join("out", "a_scene_results.mat"), os.path.join("out", "a_scene_results.png"))
    a = si.parse_args(["--ibims1", "x:y", "--ibims1_pd", "u:v"])
    assert (a.ibims1, a.ibims1_pd) == ("x:y", "u:v")
