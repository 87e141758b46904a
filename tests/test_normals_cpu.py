"""CPU: the normal rules of DESIGN.md section 23 -- the restatement's per-pixel loop, its vectorised form and the module's own numpy path
agree as bits; the cases without a normal; an analytic plane; error_stats against the exact angles of the same chords; the CPU paths of
angular_error, the accumulator, from_planes and mesh(normals=...); PLY files with normals; colorize against its formula."""
import math

import numpy as np
import pytest
import torch

import mesh_restate as M
import normals_restate as R
from planerecnet_amd import normals as N
from planerecnet_amd import reconstruct as rc

SHAPES = [(1, 1), (1, 9), (7, 1), (3, 5), (7, 9), (17, 33)]


def _module(depth, K, labels=None, **kw):
    n, ok, img = N.from_depth(torch.from_numpy(depth), K, None if labels is None else torch.from_numpy(labels), image=True, **kw)
    assert n.shape == (1,) + depth.shape + (3,) and ok.dtype == torch.bool and img.dtype == torch.uint8
    return n[0].numpy(), ok[0].numpy(), img[0].numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_loop_equals_vectorised_equals_the_numpy_path(shape):
    H, W = shape
    depth, labels, _, K = M.scene(H, W, seed=H * 100 + W, holes=0.03)
    valid_somewhere = 0
    for step in (1, 2, 3, 40):
        for relative in (True, False):
            for sign in ("camera", "plane"):
                for lab in (None, labels):
                    kw = dict(step=step, max_gap=0.5, relative=relative, sign=sign)
                    loop, vec, mod = R.normals_loop(depth, K, lab, **kw), R.normals_vec(depth, K, lab, **kw), _module(depth, K, lab, **kw)
                    assert R.same(loop, vec) and R.same(vec, mod), (shape, kw, lab is None)
                    valid_somewhere += int(vec[1].sum())
                    length = np.linalg.norm(vec[0].astype(np.float64), axis=-1)
                    assert np.all(np.abs(length[vec[1]] - 1.0) < 1e-6) and not vec[0][~vec[1]].any() and not vec[2][~vec[1]].any()
    assert (valid_somewhere > 0) == (H > 1 and W > 1)


def test_sign_and_orientation():
    depth = np.full((5, 6), 2.0, np.float32)                        # fronto-parallel: (0, 0, -1) towards the camera
    K = M.k_of(50.0, 50.0, 2.5, 2.0)
    n, ok, img = _module(depth, K)
    assert ok.all() and np.array_equal(n, np.broadcast_to(np.array([0, 0, -1], np.float32), n.shape))
    assert np.array_equal(np.unique(img.reshape(-1, 3), axis=0), [[0, 128, 128]])
    p, okp, _ = _module(depth, K, sign="plane")
    assert okp.all() and np.array_equal(p[..., 2], np.ones((5, 6), np.float32))
    with pytest.raises(ValueError):
        N.from_depth(torch.from_numpy(depth), K, sign="up")


@pytest.mark.parametrize("case", [((1, 9), 1), ((7, 1), 1), ((3, 5), 5), ((3, 5), 40), ((7, 9), 9)])
def test_no_normal_without_a_neighbour_in_both_directions(case):
    (H, W), step = case
    depth = np.full((H, W), 2.0, np.float32)
    K = M.k_of(20.0, 20.0, 0.5 * W, 0.5 * H)
    for got in (R.normals_loop(depth, K, step=step), R.normals_vec(depth, K, step=step), _module(depth, K, step=step)):
        assert not got[1].any() and not got[0].any() and not got[2].any()
    if (H, W) == (7, 9):
        assert _module(depth, K, step=8)[1].sum() == 0 and _module(depth, K, step=3)[1].all()                 # 8 >= H: no v neighbour
        assert _module(depth, K, step=6)[1].sum() == 12                                               # rows 0 and 6 of columns 0-2 and 6-8


def test_refusals_on_the_host():
    d = torch.ones(4, 6)
    K = M.k_of(5.0, 5.0, 3.0, 2.0)
    for kw in (dict(step=0), dict(step=-1), dict(step=1.5), dict(step=True), dict(max_gap=-0.1), dict(max_gap=math.inf), dict(max_gap=math.nan),
               dict(depth_range=(math.nan, 1.0))):
        with pytest.raises(ValueError):
            N.from_depth(d, K, **kw)
    with pytest.raises(RuntimeError):
        N.from_depth(d.double(), K)
    with pytest.raises(RuntimeError):
        N.from_depth(d, K, labels=torch.ones(4, 6, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        N.from_depth(torch.ones(1, 1, 4096, 4096), K)
    with pytest.raises(ValueError):
        N.angular_error(torch.zeros(3, 3), torch.ones(3, dtype=torch.bool), torch.zeros(3, 3), torch.ones(3, dtype=torch.bool), thresholds=range(9))
    with pytest.raises(ValueError):
        N.angular_error(torch.zeros(3, 3), torch.ones(3, dtype=torch.bool), torch.zeros(3, 3), torch.ones(3, dtype=torch.bool), thresholds=(181.0,))


def _plane_depth(H, W, K, n, d):
    v, u = np.mgrid[:H, :W].astype(np.float64)
    rx, ry = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    return (d / (n[0] * rx + n[1] * ry + n[2])).astype(np.float32)


def test_analytic_plane():
    """a noise-free plane n . X = d: every pixel has a normal, and its angle to n is the fp32 rounding of the depth (measured with a prototype
    of the rules: at most 0.0164 degrees; the bound is three times that)"""
    H, W = 120, 160
    K = M.scene(H, W)[3]
    n = np.array([0.3, -0.5, -0.8])
    n /= np.linalg.norm(n)
    depth = _plane_depth(H, W, K, n, -2.5)
    assert np.isfinite(depth).all() and (depth > 0).all()
    for step in (1, 3):
        got, ok, _ = _module(depth, K, step=step, max_gap=0.5)
        assert ok.all()
        angle = np.degrees(np.arccos(np.clip(got.astype(np.float64) @ n, -1.0, 1.0)))
        print("step", step, "largest angle to the true normal", angle.max())
        assert angle.max() <= 0.05
    plane, okp, _ = _module(depth, K, max_gap=0.5, sign="plane")
    assert okp.all() and np.array_equal(plane, -_module(depth, K, max_gap=0.5)[0])


@pytest.fixture(scope="module")
def pair():
    """scene normals at step 1 and at step 4: two maps whose angles spread over many bins"""
    depth, labels, _, K = M.scene(120, 160, seed=4, holes=0.01)
    a, va, _ = R.normals_vec(depth, K, None, step=1, max_gap=0.5)
    b, vb, _ = R.normals_vec(depth, K, None, step=4, max_gap=0.5)
    return a, va, b, vb


def test_error_tables_of_the_numpy_path(pair):
    a, va, b, vb = pair
    t = [torch.from_numpy(x) for x in pair]
    thresholds = (0.0, 5.0, 11.25, 22.5, 30.0, 90.0, 180.0)
    hist, within, count = N.angular_error(*t, thresholds=thresholds)
    want = R.error_tables(a, va, b, vb, thresholds)
    assert hist.shape == (1, R.BINS) and within.shape == (1, 7) and count.shape == (1,) and hist.dtype == within.dtype == count.dtype == torch.int64
    assert np.array_equal(hist[0].numpy(), want[0]) and np.array_equal(within[0].numpy(), want[1]) and int(count[0]) == int(want[2]) > 10000
    assert int(hist.sum()) == int(count[0]) and int(within[0, -1]) == int(count[0]) and N.error_bins() == R.BINS
    batch = [torch.stack([x, y]) for x, y in zip(t, (t[2], t[3], t[0], t[1]))]           # [2,H,W,...]: (a, b) and (b, a)
    h2, w2, c2 = N.angular_error(*batch, thresholds=thresholds)
    assert torch.equal(h2[0], hist[0]) and torch.equal(h2[1], hist[0]) and torch.equal(w2[1], within[0]) and c2.tolist() == [int(count[0])] * 2
    acc = N.NormalErrorAccumulator(thresholds)
    acc.add(*t).add(*batch)
    h, w, c = acc.tables()
    assert np.array_equal(h, 3 * want[0]) and np.array_equal(w, 3 * want[1]) and int(c) == 3 * int(want[2])
    res, single = acc.result(), N.error_stats(hist, within, count)
    assert res["count"] == 3 * single["count"] and res["median"] == single["median"] and res["mean"] == pytest.approx(single["mean"], rel=1e-12)


def test_error_stats_against_the_exact_angles(pair):
    a, va, b, vb = pair
    thresholds = (11.25, 22.5, 30)
    hist, within, count = R.error_tables(a, va, b, vb, thresholds)
    s = N.error_stats(hist, within, count)
    exact = R.exact_angles(a, va, b, vb)
    n = exact.size
    half = 0.5 * max(R.bin_width(int(i)) for i in np.flatnonzero(hist))
    exact_median = np.sort(exact)[(n + 1) // 2 - 1]                  # the (n + 1) // 2-th smallest: the element whose bin the histogram reports
    print("mean", s["mean"], exact.mean(), "median", s["median"], exact_median, "rmse", s["rmse"], math.sqrt((exact ** 2).mean()), "half width", half)
    assert s["count"] == n and abs(s["mean"] - exact.mean()) <= half and abs(s["median"] - exact_median) <= half
    assert abs(s["rmse"] - math.sqrt((exact ** 2).mean())) <= half
    d2 = R.squared_chords(a, va, b, vb)
    assert s["within"].tolist() == [float((d2 <= t).sum()) / n for t in R.thr2_of(thresholds)]
    assert 0.0 < s["within"][0] < s["within"][2] < 1.0
    assert R.bin_width(0) == pytest.approx(0.028, abs=1e-3) and R.bin_width(int(R.BINS / 2 * math.sqrt(2.0))) == pytest.approx(0.040, abs=1e-3)
    # torch tables with a batch axis pool; n = 0 gives NaN everywhere
    pooled = N.error_stats(torch.from_numpy(np.stack([hist, hist])), torch.from_numpy(np.stack([within, within])), torch.tensor([int(count)] * 2))
    assert pooled["count"] == 2 * n and pooled["mean"] == pytest.approx(s["mean"], rel=1e-12) and pooled["median"] == s["median"]
    empty = N.error_stats(np.zeros(R.BINS, np.int64), np.zeros(3, np.int64), 0)
    assert empty["count"] == 0 and all(math.isnan(empty[k]) for k in ("mean", "median", "rmse")) and np.isnan(empty["within"]).all()
    one = np.zeros(R.BINS, np.int64)
    one[7] = 5
    s1 = N.error_stats(one, np.array([5]), 5)
    theta7 = math.degrees(2 * math.asin(7.5 * 2 / R.BINS / 2))
    assert s1["mean"] == pytest.approx(theta7, rel=1e-12) and s1["median"] == pytest.approx(theta7, rel=1e-12) and s1["within"].tolist() == [1.0]


def test_from_planes():
    labels = torch.tensor([[0, 1, 2], [3, 4, 1]], dtype=torch.int32)
    planes = torch.tensor([[0.0, 0.0, 1.0, 2.0], [0.6, 0.0, 0.8, 1.0], [math.nan] * 4], dtype=torch.float64)      # label 3: not fitted; 4: no such plane
    n, ok = N.from_planes(labels, planes)
    assert ok.tolist() == [[False, True, True], [False, False, True]] and n.dtype == torch.float32
    assert n[0, 1].tolist() == [0.0, 0.0, -1.0] and torch.equal(n[0, 2], -planes[1, :3].float()) and not n[~ok].any()
    p, okp = N.from_planes(labels, planes, sign="plane")
    assert torch.equal(okp, ok) and torch.equal(p[ok], -n[ok])


def test_mesh_carries_the_normals_of_its_vertices(tmp_path):
    depth, labels, colors, K = M.scene(9, 14, seed=3, holes=0.1)
    d, l, c = torch.from_numpy(depth), torch.from_numpy(labels), torch.from_numpy(colors)
    n, ok, _ = N.from_depth(d, K, l, max_gap=0.5)
    plain, m = rc.mesh(d, K, l, c), rc.mesh(d, K, l, c, normals=n[0])
    assert plain.normals is None and "normals" not in plain.cpu()[0] and M.same(M.from_mesh(plain)[0], M.from_mesh(m)[0])
    nv = int(m.counts[0, 0])
    vid = m.vertex_id[0].numpy()
    assert 0 < nv < 9 * 14 and m.normals.shape == (1, 9 * 14, 3)
    assert np.array_equal(m.normals[0, :nv].numpy().view(np.uint8), n[0].numpy()[vid >= 0].view(np.uint8))
    got = m.cpu()[0]
    assert list(got) == ["vertices", "faces", "labels", "colors", "normals"] and np.array_equal(got["normals"], m.normals[0, :nv].numpy())
    cloud = rc.point_cloud(d, K, l, normals=n)
    assert cloud.faces is None and torch.equal(cloud.normals, m.normals)
    with pytest.raises(RuntimeError):
        rc.mesh(d, K, l, c, normals=n[0, :-1])


HEAD = ("ply\nformat %s 1.0\ncomment made here\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
        "property float nz\n%sproperty int label\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n")
RGB = "property uchar red\nproperty uchar green\nproperty uchar blue\n"


def _image_dict(colors=True):
    return {"vertices": np.array([[0.1, -2.5, 3.0], [1e-20, 7.25, -0.0], [3.4e38, 1.0, 2.0]], np.float32), "faces": np.array([[0, 2, 1]], np.int32),
            "labels": np.array([0, 3, -1], np.int32), "colors": np.array([[1, 2, 3], [0, 255, 7], [9, 8, 7]], np.uint8) if colors else None,
            "normals": np.array([[0.0, 0.0, -1.0], [0.26726124, -0.5345225, 0.80178374], [0.0, 0.0, 0.0]], np.float32)}


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("colors", [True, False])
def test_ply_with_normals(tmp_path, binary, colors):
    d = _image_dict(colors)
    path = str(tmp_path / "n.ply")
    rc.write_ply(path, d, binary=binary, comment="made here")
    data = open(path, "rb").read()
    head = (HEAD % ("binary_little_endian" if binary else "ascii", RGB if colors else "")).encode("ascii")
    assert data.startswith(head)
    if binary:
        per = 31 if colors else 28
        assert len(data) == len(head) + 3 * per + 13
        first = data[len(head):len(head) + per]
        assert first[:24] == d["vertices"][0].tobytes() + d["normals"][0].tobytes() and first[-4:] == d["labels"][:1].tobytes()
        assert not colors or first[24:27] == bytes([1, 2, 3])
    back = rc.read_ply(path)
    assert list(back) == ["vertices", "faces", "labels", "colors", "comments", "normals"] and back["comments"] == ["made here"]
    for key in ("vertices", "faces", "labels", "colors", "normals"):
        if d[key] is None:
            assert back[key] is None
        else:
            assert back[key].dtype == d[key].dtype and back[key].tobytes() == d[key].tobytes(), key
    # without normals the file is the one it always was
    plain = dict(d)
    del plain["normals"]
    p0, p1 = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    rc.write_ply(p0, plain, binary=binary)
    rc.write_ply(p1, dict(plain, normals=None), binary=binary)
    old = open(p0, "rb").read()
    assert old == open(p1, "rb").read() and b"nx" not in old and "normals" not in rc.read_ply(p0)
    assert not binary or len(old) == len(rc._header(True, [], 3, colors, 1)) + 3 * (per - 12) + 13
    with pytest.raises(ValueError):
        rc.write_ply(p1, dict(d, normals=d["normals"][:2]), binary=binary)


def test_read_ply_still_refuses_what_write_ply_does_not_make(tmp_path):
    d = _image_dict(True)
    path = str(tmp_path / "n.ply")
    rc.write_ply(path, d, binary=False)
    good = open(path, "rb").read()
    assert rc.read_ply(path)["normals"].shape == (3, 3)
    nl = b"property float nx\nproperty float ny\nproperty float nz\n"
    assert good.count(nl) == 1
    bad = {"normals after the colours": good.replace(nl, b"").replace(b"property int label\n", nl + b"property int label\n"),
           "a lone nx after label": good.replace(nl, b"").replace(b"property int label\n", b"property int label\nproperty float nx\n"),
           "two of three": good.replace(b"property float nz\n", b""),
           "wrong order": good.replace(nl, b"property float ny\nproperty float nx\nproperty float nz\n"),
           "double type": good.replace(b"property float nx", b"property double nx"),
           "a row without its normal": good.replace(b" 0 0 -1 ", b" ", 1),
           "a word for a number": good.replace(b" 0 0 -1 ", b" 0 up -1 ", 1)}
    for why, data in bad.items():
        assert data != good, why
        with open(path, "wb") as f:
            f.write(data)
        with pytest.raises(ValueError):
            rc.read_ply(path)
    rc.write_ply(path, d, binary=True)
    data = open(path, "rb").read()
    for cut in (data[:-1], data + b"\0", data[:-12]):
        with open(path, "wb") as f:
            f.write(cut)
        with pytest.raises(ValueError):
            rc.read_ply(path)


def test_colorize_against_the_formula():
    ties = [np.float32((2 * k + 1) / 255.0 - 1.0) for k in (0, 1, 63, 126, 127, 128, 254)]     # the fp32 values nearest a byte boundary
    vals = [-1.0, 0.0, -0.0, 1.0, 1e-30, -1e-30, 0.5, -0.5, 0.999999, -0.999999] + ties + [np.nextafter(t, np.float32(2)) for t in ties] + \
           [np.nextafter(t, np.float32(-2)) for t in ties]
    vals = np.array(vals, np.float32)
    want = np.array([round((float(v) * 0.5 + 0.5) * 255.0) for v in vals], np.uint8)     # Python rounds halves to even, as rint does
    assert want[0] == 0 and want[1] == 128 and want[3] == 255 and want[4] == want[5] == 128          # 127.5 -> 128: the one exact tie
    n = np.zeros((len(vals), 2, 3), np.float32)
    n[:, 0, 0], n[:, 0, 1], n[:, 0, 2] = vals, vals[::-1], -vals
    n[:, 1] = n[:, 0]
    valid = np.ones((len(vals), 2), bool)
    valid[:, 1] = False
    expect = np.zeros((len(vals), 2, 3), np.uint8)
    expect[:, 0, 2], expect[:, 0, 1] = want, want[::-1]
    expect[:, 0, 0] = [round((float(-v) * 0.5 + 0.5) * 255.0) for v in vals]
    assert np.array_equal(N.colorize(n, valid), expect)
    got = N.colorize(torch.from_numpy(n), torch.from_numpy(valid))
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), expect)
    depth, labels, _, K = M.scene(17, 33, seed=2, holes=0.05)
    a, va, img = N.from_depth(torch.from_numpy(depth), K, torch.from_numpy(labels), max_gap=0.5, image=True)
    assert va.any() and torch.equal(N.colorize(a, va), img) and np.array_equal(N.colorize(a.numpy(), va.numpy()), img.numpy())
