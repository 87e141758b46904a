"""CPU: greedy mask NMS -- the numpy restatements (tests/mask_nms_restate.py) and nms.mask_nms on CPU tensors against the keep vectors of
the real reference (tests/golden/mask_nms.npz), and the host-side half of prn_mask_nms (argument validation before any launch, workspace
size)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mask_nms_restate as R


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "mask_nms.npz"))


@pytest.fixture(scope="module")
def cases():
    return R.cases()


def test_fixture_holds_every_case_and_the_generators_did_not_drift(fixture, cases):
    assert sorted(fixture.files) == sorted(p + k for k in cases for p in ("keep_", "area_"))
    for name, (labels, masks, sums, thr) in cases.items():
        assert np.array_equal(fixture["area_" + name], masks.reshape(len(masks), -1).sum(1)), name
        assert fixture["keep_" + name].shape == labels.shape
    for name, v in R.hand_cases().items():
        assert np.array_equal(fixture["keep_" + name], v[4]), name                     # what the arithmetic gives by hand


def test_restatements_equal_the_reference(fixture, cases):
    for name, (labels, masks, sums, thr) in cases.items():
        assert np.array_equal(R.reference_loop(labels, masks, sums, thr), fixture["keep_" + name]), name
        assert np.array_equal(R.row_vectorised(labels, masks, sums, thr), fixture["keep_" + name]), name


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8])
def test_host_mask_nms_equals_the_reference(fixture, cases, dtype):
    from planerecnet_amd import nms
    for name, (labels, masks, sums, thr) in cases.items():
        n = len(labels)
        keep = nms.mask_nms(torch.from_numpy(labels), torch.from_numpy(masks).to(dtype), torch.from_numpy(sums), torch.linspace(0.9, 0.1, n), nms_thr=thr)
        assert keep.dtype == dtype and not keep.is_cuda
        assert np.array_equal(keep.numpy().astype(np.uint8), fixture["keep_" + name]), name
    assert nms.mask_nms(torch.zeros(0, dtype=torch.long), torch.zeros(0, 4, 4, dtype=dtype), torch.zeros(0), torch.zeros(0)) == []


def test_batched_call_refuses_cpu_tensors():
    from planerecnet_amd import nms
    with pytest.raises(RuntimeError, match="device tensors"):
        nms.mask_nms_batched(torch.zeros(2, dtype=torch.long), torch.ones(2, 4, 4, dtype=torch.bool), torch.full((2,), 16.0), [2])


def test_entry_point_validates_before_any_launch():
    """Every refusal listed in include/prn.h: rc != 0 and a message, with pointers nothing could dereference (no GPU here)."""
    from planerecnet_amd import _lib
    lib = _lib.lib
    p = ctypes.c_void_p(4096)
    err = lambda: lib.prn_last_error().decode()      # noqa: E731

    def call(masks=p, labels=p, sums=p, seg=p, n_img=1, n_max=8, HW=64, keep=p, ws=p):
        return lib.prn_mask_nms(masks, labels, sums, seg, n_img, n_max, HW, 0.5, keep, ws, None)
    for name in ("masks", "labels", "sums", "seg", "keep", "ws"):
        assert call(**{name: None}) != 0 and "null" in err(), name
    assert call(n_img=0) != 0 and "n_img" in err()
    assert call(n_img=-3) != 0 and "n_img" in err()
    assert call(n_max=0) != 0 and "n_max" in err()
    limit = 4096
    assert call(n_max=limit + 1) != 0 and "n_max" in err() and str(limit) in err()
    assert call(HW=1 << 24) != 0 and "2^24" in err()
    assert call(HW=0) != 0 and "2^24" in err()
    from planerecnet_amd import nms
    assert nms.MASK_NMS_MAX == limit
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "prn.h")).read()
    assert "#define PRN_MASK_NMS_MAX %d" % limit in header


def test_workspace_size_is_monotone_in_each_argument():
    from planerecnet_amd import _lib
    ws = _lib.lib.prn_mask_nms_ws_bytes
    base = (300, 100, 19200)
    for k, values in enumerate(((1, 2, 63, 64, 65, 300, 4096, 32768), (1, 63, 64, 65, 128, 129, 4096), (1, 31, 32, 33, 64, 19200, (1 << 24) - 1))):
        sizes = []
        for v in values:
            a = list(base)
            a[k] = v
            sizes.append(ws(*a))
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (k, sizes)
        assert sizes[-1] > sizes[0]
    # the packed bits (one bit per pixel, whole 32-bit words) and one 64-bit word per candidate and block of 64 candidates both fit
    assert ws(500, 500, 19200) >= 500 * 600 * 4 + 500 * 8 * 8
    assert ws(4096, 4096, 64) >= 4096 * 2 * 4 + 4096 * 64 * 8
