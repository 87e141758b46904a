"""CPU: connected components and mask cleaning (planerecnet_amd/components.py) -- scipy.ndimage's answers stored in
tests/golden/components_cases.npz through both numpy restatements (tests/components_restate.py) and through the module's host path, random
masks against scipy directly where it is installed, the argument errors, and the new flags of simple_inference.py.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import components_restate as R

NAMES = ("count", "kept", "largest", "area")


def _components():
    from planerecnet_amd import components
    return components


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return R.load_fixture(os.path.join(golden_dir, "components_cases.npz"))


def test_fixture_holds_the_hand_made_cases(fixture):
    assert sorted(fixture) == ["a", "b"]
    for tag, c in fixture.items():
        H, W = c["masks"].shape[1:]
        P = R.patterns(H, W, densities=(0.1, 0.5, 0.59, 0.9) if tag == "a" else ())
        assert sorted(P) == c["names"]
        for n, name in enumerate(c["names"]):
            assert np.array_equal(P[name], c["masks"][n]), name
        k = {name: (int(c["count"][4][n]), int(c["count"][8][n])) for n, name in enumerate(c["names"])}
        assert k["empty"] == (0, 0) and k["full"] == (1, 1) and k["corners"] == (4, 4)
        assert k["diagonal"] == (min(H, W), 1) and k["checker"] == ((H * W + 1) // 2, 1)
        assert k["serpentine"] == (1, 1) and k["serpentine_v"] == (1, 1) and k["spiral"] == (1, 1)
        assert k["ucorner"] == (2, 1) and k["ucorner_anti"] == (2, 1)                 # the corner neighbour joins for 8 only
        assert k["tie2"] == (3, 3) and k["tie3"] == (4, 4)


@pytest.mark.parametrize("connectivity", (4, 8))
def test_both_restatements_agree_with_the_fixture(fixture, connectivity):
    for tag, c in fixture.items():
        want, cnt = c["labels"][connectivity], c["count"][connectivity]
        got, k = R.label_minprop(c["masks"], connectivity)
        assert np.array_equal(got, want) and np.array_equal(k, cnt), tag
        for n, name in enumerate(c["names"]):
            lab, kf = R.label_flood(c["masks"][n], connectivity)
            assert kf == cnt[n] and np.array_equal(lab, want[n]), (tag, name)
        for v, (keep, min_area, fill) in enumerate(R.CLEAN_VARIANTS):
            for label in ((R.label_minprop, R.label_flood) if tag == "a" else (R.label_flood,)):      # (minimum propagation is slow on long chains)
                got, info = R.clean_batch(c["masks"], connectivity, keep, min_area, fill, label=label)
                assert np.array_equal(got, c["clean"][connectivity, v]), (tag, v)
                assert np.array_equal(np.stack([info[k] for k in NAMES]), c["info"][connectivity, v]), (tag, v)


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("dtype", (torch.bool, torch.uint8))
def test_host_path_equals_the_fixture(fixture, connectivity, dtype):
    C = _components()
    for tag, c in fixture.items():
        m = torch.from_numpy(c["masks"])
        if dtype == torch.uint8:
            m = m.to(torch.uint8) * 200                                                 # non-zero = set
        before = m.clone()
        labels, count = C.label(m, connectivity)
        assert labels.dtype == torch.int32 and count.dtype == torch.int32 and labels.shape == m.shape
        assert np.array_equal(labels.numpy(), c["labels"][connectivity]) and np.array_equal(count.numpy(), c["count"][connectivity])
        for v, (keep, min_area, fill) in enumerate(R.CLEAN_VARIANTS):
            out, info = C.clean(m, connectivity, keep=keep, min_area=min_area, fill_holes=fill)
            assert out.dtype == dtype and out.shape == m.shape
            assert np.array_equal(out.numpy() != 0, c["clean"][connectivity, v]), (tag, v)
            assert int(out.max()) <= 1
            assert np.array_equal(np.stack([info[k].numpy() for k in NAMES]), c["info"][connectivity, v]), (tag, v)
        assert torch.equal(m, before)


def test_ties_min_area_and_the_speck_in_a_hole(fixture):
    """the rules the fixture's numbers stand for, spelled out on the host path"""
    C = _components()
    c = fixture["a"]
    at = {name: torch.from_numpy(c["masks"][n:n + 1]) for n, name in enumerate(c["names"])}
    for name in ("tie2", "tie3"):
        out, info = C.clean(at[name], 8)
        lab, _ = R.label_flood(at[name][0].numpy(), 8)
        assert np.array_equal(out[0].numpy(), lab == 2) and int(info["largest"][0]) == 6 and int(info["area"][0]) == 6      # label 1 is the smaller speck
    for min_area, kept_all, kept_largest in ((5, 1, 1), (6, 1, 1), (7, 0, 0)):
        _, info = C.clean(at["areas_6_4_1"], 8, keep="all", min_area=min_area)
        assert (int(info["count"][0]), int(info["kept"][0]), int(info["largest"][0])) == (3, kept_all, 6)
        out, info = C.clean(at["areas_6_4_1"], 8, keep="largest", min_area=min_area)
        assert int(info["kept"][0]) == kept_largest and int(info["area"][0]) == 6 * kept_largest and bool(out.any()) == bool(kept_largest)
    H, W = c["masks"].shape[1:]
    out, info = C.clean(at["speck_in_hole"], 8, keep="largest", fill_holes=True)       # the speck goes first, then the whole hole fills
    assert int(info["area"][0]) == (H - 2) * (W - 2) and bool(out[0, H // 2, W // 2])
    out, info = C.clean(at["speck_in_hole"], 8, keep="all", fill_holes=True)
    assert int(info["area"][0]) == (H - 2) * (W - 2) and int(info["kept"][0]) == 2
    out, _ = C.clean(at["open_hole"], 8, keep="all", fill_holes=True)                   # a hole that reaches the border is none
    assert torch.equal(out, at["open_hole"])


def test_random_masks_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    C = _components()
    cross, full = ndimage.generate_binary_structure(2, 1), np.ones((3, 3), bool)
    rng = np.random.RandomState(5)
    ties = 0
    for case in range(60):
        H, W = int(rng.randint(1, 48)), int(rng.randint(1, 64))
        m = rng.rand(2, H, W) < rng.choice([0.1, 0.3, 0.5, 0.59, 0.9])
        for conn in (4, 8):
            fg, dual = (full, cross) if conn == 8 else (cross, full)
            keep, min_area, fill = ("largest", "all")[case % 2], int(rng.randint(0, 8)), bool(case % 3)
            labels, count = C.label(torch.from_numpy(m), conn)
            out, info = C.clean(torch.from_numpy(m), conn, keep=keep, min_area=min_area, fill_holes=fill)
            for n in range(2):
                lab, K = ndimage.label(m[n], structure=fg)
                assert K == int(count[n]) and np.array_equal(lab, labels[n].numpy())
                assert np.array_equal(R.label_flood(m[n], conn)[0], lab) and np.array_equal(R.label_minprop(m[n], conn)[0], lab)
                areas = np.bincount(lab.ravel(), minlength=K + 1)[1:]
                ties += int(K > 1 and (areas == areas.max()).sum() > 1)
                if keep == "largest":
                    chosen = [int(np.argmax(areas)) + 1] if K and areas.max() >= min_area else []
                else:
                    chosen = (np.flatnonzero(areas >= min_area) + 1).tolist()
                sel = np.isin(lab, chosen)
                if fill:
                    sel = ndimage.binary_fill_holes(sel, structure=dual)
                assert np.array_equal(out[n].numpy(), sel), (case, conn, keep, min_area, fill)
                assert [int(info[k][n]) for k in NAMES] == [K, len(chosen), int(areas.max()) if K else 0, int(sel.sum())]
    assert ties > 0                                                                     # the tie rule was exercised


def test_lists_none_and_empty_images_on_the_host():
    C = _components()
    rng = np.random.RandomState(2)
    parts = [torch.from_numpy(rng.rand(n, 9, 11) < 0.5) for n in (3, 0, 1)]
    masks = [parts[0], None, parts[1], parts[2]]
    labels, count = C.label(masks, 4)
    out, info = C.clean(masks, 4, keep="all", min_area=2, fill_holes=True)
    assert labels[1] is None and out[1] is None and count[1].numel() == 0 and info["area"][1].numel() == 0
    assert labels[2].shape == (0, 9, 11) and out[2].shape == (0, 9, 11) and count[2].numel() == 0
    for b, p in ((0, parts[0]), (3, parts[2])):
        l1, c1 = C.label(p, 4)
        o1, i1 = C.clean(p, 4, keep="all", min_area=2, fill_holes=True)
        assert torch.equal(labels[b], l1) and torch.equal(count[b], c1) and torch.equal(out[b], o1)
        assert all(torch.equal(info[k][b], i1[k]) for k in NAMES)
        want, winfo = R.clean_batch(p.numpy(), 4, "all", 2, True)
        assert np.array_equal(o1.numpy(), want) and np.array_equal(i1["area"].numpy(), winfo["area"])
    nothing, ninfo = C.clean([None, None])
    assert nothing == [None, None] and all(t.numel() == 0 for t in ninfo["count"])


def test_bad_arguments_raise_with_what_was_seen():
    C = _components()
    m = torch.zeros(2, 4, 5, dtype=torch.bool)
    for conn in (6, 0, "8"):
        with pytest.raises(RuntimeError, match="connectivity"):
            C.label(m, conn)
        with pytest.raises(RuntimeError, match="connectivity"):
            C.clean(m, conn)
    with pytest.raises(RuntimeError, match="keep"):
        C.clean(m, keep="biggest")
    for bad in (-1, 2.5):
        with pytest.raises(RuntimeError, match="min_area"):
            C.clean(m, min_area=bad)
    with pytest.raises(RuntimeError, match=r"float32.*\(2, 4, 5\)"):
        C.label(m.float())
    with pytest.raises(RuntimeError, match=r"\(4, 5\)"):
        C.clean(m[0])
    with pytest.raises(RuntimeError, match=r"masks\[1\]"):
        C.label([m, m.to(torch.uint8)])                                                 # mixed dtypes
    with pytest.raises(RuntimeError, match=r"masks\[1\]"):
        C.clean([m, torch.zeros(1, 4, 6, dtype=torch.bool)])                            # mixed sizes
    with pytest.raises(RuntimeError, match="masks"):
        C.label([m, "x"])
    if torch.cuda.is_available():
        with pytest.raises(RuntimeError, match=r"masks\[1\]"):
            C.label([m, m.cuda()])                                                      # mixed devices


def test_library_refuses_bad_sizes_on_the_host():
    """validation precedes every launch: checked here without a GPU"""
    import ctypes
    from planerecnet_amd import _lib
    lib = _lib.lib
    assert lib.prn_ccl_ws_bytes(3, 480, 640) >= 3 * 480 * 640 * 4
    assert lib.prn_ccl_ws_bytes(3, 480, 640) <= 3 * 480 * 640 * 4 + 3 * 4096
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (65536, 4, 4), (1, 1 << 16, 1 << 15), (1, 46341, 46341)):
        assert lib.prn_ccl_ws_bytes(*bad) == -1, bad
    assert lib.prn_ccl_ws_bytes(65535, 1, 1) > 0 and lib.prn_ccl_ws_bytes(1, 46340, 46340) > 0
    p = ctypes.c_void_p(4096)                                                           # (never dereferenced)
    rc = lib.prn_ccl_label(p, p, 1, 1, 1 << 16, 1 << 15, 8, p, p, p, None)
    assert rc != 0 and b"2^31" in lib.prn_last_error()
    rc = lib.prn_ccl_clean(p, p, 1, 65536, 4, 4, 8, 0, 0, 0, p, p, p, p, p, p, None)
    assert rc != 0 and b"65535" in lib.prn_last_error()
    rc = lib.prn_ccl_label(p, p, 1, 1, 4, 4, 6, p, p, p, None)
    assert rc != 0 and b"connectivity" in lib.prn_last_error()
    rc = lib.prn_ccl_clean(p, p, 1, 1, 4, 4, 8, 0, -1, 0, p, p, p, p, p, p, None)
    assert rc != 0 and b"min_area" in lib.prn_last_error()
    rc = lib.prn_ccl_clean(p, p, 1, 1, 4, 4, 8, 0, 0, 0, None, p, p, p, p, p, None)
    assert rc != 0 and b"null" in lib.prn_last_error()


def test_inference_flags_default_to_off():
    import simple_inference as si
    a = si.parse_args([])
    assert (a.clean_masks, a.min_area, a.fill_holes, a.connectivity) == ("off", 0, False, 8)
    assert si.clean_options() is None
    same = [{"pred_masks": None}]
    assert si.cleaned(same) is same                                                     # off: the results pass through untouched
    a = si.parse_args(["--clean_masks", "largest", "--min_area", "50", "--fill_holes", "--connectivity", "4"])
    assert si.clean_options() == {"keep": "largest", "min_area": 50, "fill_holes": True, "connectivity": 4}
    assert si.parse_args(["--clean_masks", "all"]).clean_masks == "all"
    for bad in (["--clean_masks", "some"], ["--connectivity", "6"], ["--min_area", "-3"]):
        with pytest.raises(SystemExit):
            si.parse_args(bad)
    si.parse_args([])
