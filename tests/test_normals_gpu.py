"""GPU: surface normals on the device (csrc/prn_normals.hip through planerecnet_amd.normals) against the numpy restatement
(tests/normals_restate.py), exactly -- normals, validity and picture compared as bits -- at sizes that straddle every launch shape (read from
the library's exported constant), over validity patterns, the gap rule on its boundary, label seams, depth extremes, batches, determinism,
untouched inputs, no host synchronisation and library refusals with real buffers; the error tables of prn_normal_error against np.bincount;
the mesh's vertex normals; eval.py's normal metrics through a stub network; simple_inference.py's normal picture and PLY normals."""
import ctypes
import io
import math
import random
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import mesh_restate as M
import normals_restate as R

pytestmark = pytest.mark.gpu


def _n():
    from planerecnet_amd import normals
    return normals


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _check(depth, K, labels=None, **kw):
    """one image on the device == the restatement, bit for bit (normals, validity, picture); -> the restatement's triple"""
    n, ok, img = _n().from_depth(_t(depth), K, _t(labels), image=True, **kw)
    assert n.shape == (1,) + depth.shape + (3,) and n.dtype == torch.float32 and ok.dtype == torch.bool and img.dtype == torch.uint8 and n.is_cuda
    want = R.normals_vec(depth, K, labels, **kw)
    got = (n[0].cpu().numpy(), ok[0].cpu().numpy(), img[0].cpu().numpy())
    assert np.array_equal(got[1], want[1]), (depth.shape, kw, int(got[1].sum()), int(want[1].sum()))
    bad = np.flatnonzero((_bits(got[0]).reshape(-1, 12) != _bits(want[0]).reshape(-1, 12)).any(1))
    assert bad.size == 0, (depth.shape, kw, bad.size, got[0].reshape(-1, 3)[bad[:3]], want[0].reshape(-1, 3)[bad[:3]])
    assert np.array_equal(got[2], want[2]), (depth.shape, kw)
    assert R.same(got, want)
    return want


def _shapes():
    px = _n().block_pixels()
    assert px % 2 == 0 and px >= 128
    return [(3, 5), (2, px // 2), (1, px), (1, px + 1), (3, px // 2), (5, 64), (4, 65), (17, px + 1)]


@pytest.mark.parametrize("which", range(8))
def test_sizes_that_straddle_the_launch_shapes(which):
    H, W = _shapes()[which]
    depth, labels, _, K = M.scene(H, W, seed=which, holes=0.01)
    for step in (1, 2, 3):
        want = _check(depth, K, step=step, max_gap=0.5)
        _check(depth, K, labels, step=step, max_gap=0.5, sign="plane", relative=False)
        print((H, W), "step", step, "valid", int(want[1].sum()))
        if which >= 5 or (which == 4 and step == 1):
            assert want[1].sum() > 0


def _slope(H, W):
    """a smooth curved surface, valid everywhere, whose one-sided and central tangents differ"""
    v, u = np.mgrid[:H, :W].astype(np.float64)
    return (2.0 + 0.03 * u + 0.02 * v + 0.001 * u * u + 0.002 * v * v + 0.0015 * u * v).astype(np.float32), M.k_of(0.9 * W + 0.37, 0.9 * W - 0.21, 0.5 * W - 0.4, 0.5 * H + 0.3)


PATTERNS = ["all", "nan", "checkerboard", "one column", "alternate rows", "holes"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_validity_patterns(pattern):
    px = _n().block_pixels()
    H, W = 37, 65
    assert H * W > 3 * px and (H * W) % px
    depth, K = _slope(H, W)
    v, u = np.mgrid[:H, :W]
    if pattern == "nan":
        depth[:] = np.nan
    elif pattern == "checkerboard":
        depth[(v + u) % 2 == 1] = np.nan
    elif pattern == "one column":
        depth[u != 7] = np.inf
    elif pattern == "alternate rows":
        depth[v % 2 == 1] = 0.0
    elif pattern == "holes":
        depth[np.random.RandomState(0).rand(H, W) < 0.05] = -1.0
    for step in (1, 2):
        want = _check(depth, K, step=step, max_gap=0.5)
        nv = int(want[1].sum())
        if pattern == "all":
            assert nv == H * W                                       # the borders and corners included: one-sided tangents
        elif pattern in ("nan", "one column"):
            assert nv == 0
        elif pattern == "checkerboard":
            assert nv == (0 if step == 1 else ((v + u) % 2 == 0).sum())      # step 1: no normal anywhere; step 2 stays on one colour
        elif pattern == "alternate rows":
            assert nv == (0 if step == 1 else ((H + 1) // 2) * W)
        else:
            assert 0 < nv < H * W


def test_holes_force_each_one_sided_tangent():
    """one hole: its four neighbours lose one side each and keep their normal, which differs from the one the full surface gives them"""
    H, W = 9, 11
    full, K = _slope(H, W)
    n_full = _check(full, K, max_gap=0.5)
    holed = full.copy()
    holed[4, 5] = np.nan
    want = _check(holed, K, max_gap=0.5)
    loop = R.normals_loop(holed, K, max_gap=0.5)
    assert R.same(want, loop)
    assert not want[1][4, 5] and want[1].sum() == H * W - 1
    for q in ((4, 4), (4, 6), (3, 5), (5, 5)):                      # lost E, W, S, N
        assert want[1][q] and not np.array_equal(want[0][q], n_full[0][q])
    assert np.array_equal(want[0][2, 2], n_full[0][2, 2])
    both = full.copy()                                              # a pixel between two holes in a row has no tangent along u
    both[4, 4] = both[4, 6] = np.nan
    assert not _check(both, K, max_gap=0.5)[1][4, 5]
    assert _check(both.T.copy(), K, max_gap=0.5)[1][5, 4] == False  # noqa: E712  (... and along v)


def test_gap_rule_on_its_boundary():
    up = np.nextafter(np.float32(2.5), np.float32(3.0))
    K = M.k_of(2.0, 2.0, 0.5, 0.5)
    for relative, gap in ((True, 0.25), (False, 0.5)):
        at = _check(np.array([[2.0, 2.5], [2.0, 2.0]], np.float32), K, max_gap=gap, relative=relative)          # 0.5 <= 0.5 is exact: usable
        assert at[1].all()
        above = _check(np.array([[2.0, up], [2.0, 2.0]], np.float32), K, max_gap=gap, relative=relative)
        assert above[1].tolist() == [[False, False], [True, False]]


def test_label_seam():
    H, W = 12, 20
    depth, K = _slope(H, W)
    labels = np.where(np.mgrid[:H, :W][1] < 9, 1, 2).astype(np.int32)
    on = _check(depth, K, labels, max_gap=0.5)
    off = _check(depth, K, labels, max_gap=0.5, same_label=False)
    none = _check(depth, K, None, max_gap=0.5)
    assert on[1].all() and R.same(off, none)
    differs = (on[0] != off[0]).any(-1)
    assert differs[:, 8:10].all() and not differs[:, :8].any() and not differs[:, 10:].any()       # the seam's two columns went one-sided
    lone = labels.copy()
    lone[5, 5] = 7                                                  # a pixel of its own label has no usable neighbour
    assert not _check(depth, K, lone, max_gap=0.5)[1][5, 5]
    depth2, labels2, _, K2 = M.scene(37, 65, seed=8, holes=0.02)
    for kw in (dict(), dict(same_label=False), dict(max_gap=0.5, step=2), dict(depth_range=(1.5, 3.0), max_gap=0.5), dict(max_gap=0.0)):
        _check(depth2, K2, labels2, **kw)


def test_depth_extremes():
    K = M.k_of(3.0, 3.2, 1.1, 0.9)
    v, u = np.mgrid[:3, :4]
    for base in (1e-30, 3.4e38 / 1.5):
        depth = (np.float32(base) * (1.0 + 0.01 * u + 0.02 * v)).astype(np.float32)
        want = _check(depth, K, max_gap=3.0e38)                      # (relative: the bound overflows to inf, which is no limit)
        assert want[1].all()
    mixed = np.where((v + u) % 2 == 0, np.float32(1e-30), np.float32(3.4e38)).astype(np.float32)
    _check(mixed, K, max_gap=3.0e38)
    _check(mixed, K, max_gap=3.0e38, relative=False)


@pytest.fixture(scope="module")
def big():
    """the 480 x 640 scene and its restated normals at steps 1 and 3, computed once"""
    depth, labels, _, K = M.scene(480, 640, seed=1, holes=0.01)
    return depth, labels, K, {s: R.normals_vec(depth, K, labels, step=s) for s in (1, 3)}


@pytest.mark.parametrize("step", [1, 3])
def test_480_by_640(big, step):
    depth, labels, K, want = big
    n, ok, img = _n().from_depth(_t(depth), K, _t(labels), step=step, image=True)
    got = (n[0].cpu().numpy(), ok[0].cpu().numpy(), img[0].cpu().numpy())
    print("step", step, "valid", int(got[1].sum()))
    assert np.array_equal(got[1], want[step][1]) and R.same(got, want[step])
    assert got[1].sum() > 290000


def test_batch_determinism_and_untouched_inputs():
    N = _n()
    H, W = 37, 65
    scenes = [M.scene(H, W, seed=s, holes=0.05 * s) for s in range(3)]
    scenes[1][0][:] = np.nan
    Ks = np.stack([s[3] * np.array([[1.0 + 0.1 * i, 1, 1], [1, 1.0 - 0.05 * i, 1], [1, 1, 1]]) for i, s in enumerate(scenes)])
    d = _t(np.stack([s[0] for s in scenes]))[:, None]
    lab = _t(np.stack([s[1] for s in scenes]))
    keep = (d.clone(), lab.clone())
    n, ok, img = N.from_depth(d, Ks, lab, max_gap=0.5, image=True)
    n2, ok2, img2 = N.from_depth(d, Ks, lab, max_gap=0.5, image=True)
    assert n.shape == (3, H, W, 3) and torch.equal(n.view(torch.int32), n2.view(torch.int32)) and torch.equal(ok, ok2) and torch.equal(img, img2)
    assert not ok[1].any() and ok[0].any() and ok[2].any()
    for b in range(3):
        nb, okb, imgb = N.from_depth(d[b], torch.from_numpy(Ks[b]).cuda(), lab[b], max_gap=0.5, image=True)
        assert torch.equal(nb[0].view(torch.int32), n[b].view(torch.int32)) and torch.equal(okb[0], ok[b]) and torch.equal(imgb[0], img[b])
        want = R.normals_vec(scenes[b][0], Ks[b], scenes[b][1], max_gap=0.5)
        assert R.same((n[b].cpu().numpy(), ok[b].cpu().numpy(), img[b].cpu().numpy()), want)
    assert torch.equal(d.view(torch.int32), keep[0].view(torch.int32)) and torch.equal(lab, keep[1])
    assert N.from_depth(d, Ks, lab)[2] is None


def _unit(n, seed):
    rng = np.random.RandomState(seed)
    a = rng.randn(n, 3)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = a + 0.3 * rng.randn(n, 3) * rng.rand(n, 1)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return a.astype(np.float32), rng.rand(n) < 0.9, b.astype(np.float32), rng.rand(n) < 0.9


THRESHOLDS = (0.0, 11.25, 22.5, 30.0, 180.0)


def _error_check(a, va, b, vb, thresholds=THRESHOLDS):
    hist, within, count = _n().angular_error(_t(a), _t(va), _t(b), _t(vb), thresholds=thresholds)
    assert hist.is_cuda and hist.dtype == within.dtype == count.dtype == torch.int64 and hist.shape == (1, R.BINS) and within.shape == (1, len(thresholds))
    want = R.error_tables(a, va, b, vb, thresholds)
    assert int(count[0]) == int(want[2]) and np.array_equal(within[0].cpu().numpy(), want[1])
    assert np.array_equal(hist[0].cpu().numpy(), want[0]), np.flatnonzero(hist[0].cpu().numpy() != want[0])[:8]
    return want


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097])
def test_angular_error_sizes(n):
    want = _error_check(*_unit(n, seed=n))
    assert n == 1 or (0 < want[2] <= n and want[1][-1] == want[2] and want[0].sum() == want[2])


def test_angular_error_480_by_640(big):
    _, _, _, want = big
    a, va, _ = want[1]
    b, vb, _ = want[3]
    tables = _error_check(a, va, b, vb)
    assert tables[2] > 290000 and (tables[0] > 0).sum() > 100
    N = _n()
    stats = N.error_stats(*N.angular_error(_t(a), _t(va), _t(b), _t(vb)))
    exact = R.exact_angles(a, va, b, vb)
    half = 0.5 * max(R.bin_width(int(i)) for i in np.flatnonzero(tables[0]))
    print("mean", stats["mean"], exact.mean(), "median", stats["median"], np.sort(exact)[(exact.size + 1) // 2 - 1])
    assert abs(stats["mean"] - exact.mean()) <= half and abs(stats["median"] - np.sort(exact)[(exact.size + 1) // 2 - 1]) <= half


def test_angular_error_edges():
    N = _n()
    n = 1000
    a, va, _, _ = _unit(n, seed=1)
    ones = np.ones(n, bool)
    same = _error_check(a, ones, a, ones)
    assert same[0][0] == n and same[0][1:].sum() == 0 and same[1].tolist() == [n] * 5               # bin 0; 0 degrees counts them
    up = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    opposite = _error_check(up, ones, -up, ones)
    assert opposite[0][R.BINS - 1] == n and opposite[1].tolist() == [0, 0, 0, 0, n]                 # chord 2: the clamp; 180 degrees counts them
    tilt = np.tile(np.array([math.sin(0.2), 0, math.cos(0.2)], np.float32), (n, 1))
    one_bin = _error_check(up, va, tilt, ones)
    assert (one_bin[0] > 0).sum() == 1 and one_bin[0].max() == va.sum() and one_bin[1].tolist() == [0, 0, int(va.sum()), int(va.sum()), int(va.sum())]
    none = _error_check(up, np.zeros(n, bool), tilt, ones)
    assert none[2] == 0 and none[0].sum() == 0
    hist, within, count = N.angular_error(_t(up), _t(ones), _t(tilt), _t(ones), thresholds=())
    assert within.shape == (1, 0) and int(count[0]) == n
    # B = 3, as [B,H,W,3] maps: each image its own tables; the accumulator pools them, and a second add doubles them
    sets = [_unit(24 * 40, seed=s) for s in (5, 6, 7)]
    batch = [_t(np.stack([s[i] for s in sets]).reshape((3, 24, 40, 3) if i % 2 == 0 else (3, 24, 40))) for i in range(4)]
    hist, within, count = N.angular_error(*batch, thresholds=THRESHOLDS)
    want = [R.error_tables(*s, THRESHOLDS) for s in sets]
    for b in range(3):
        assert np.array_equal(hist[b].cpu().numpy(), want[b][0]) and np.array_equal(within[b].cpu().numpy(), want[b][1]) and int(count[b]) == int(want[b][2])
    again = N.angular_error(*batch, thresholds=THRESHOLDS)
    assert all(torch.equal(x, y) for x, y in zip((hist, within, count), again))
    acc = N.NormalErrorAccumulator(THRESHOLDS, device="cuda")
    acc.add(*batch)
    h1, w1, c1 = acc.tables()
    assert np.array_equal(h1, sum(w[0] for w in want)) and np.array_equal(w1, sum(w[1] for w in want)) and int(c1) == sum(int(w[2]) for w in want)
    acc.add(*batch)
    h2, w2, c2 = acc.tables()
    assert np.array_equal(h2, 2 * h1) and np.array_equal(w2, 2 * w1) and int(c2) == 2 * int(c1)
    assert acc.result()["median"] == N.error_stats(h1, w1, c1)["median"]


def test_no_host_synchronisation():
    """Fails on a host implementation: that one downloads the depth."""
    from planerecnet_amd import reconstruct
    N = _n()
    depth, labels, colors, K = M.scene(37, 65, seed=7, holes=0.02)
    d, l, c = _t(depth), _t(labels), _t(colors)
    k_dev = torch.from_numpy(K).cuda()
    acc = N.NormalErrorAccumulator(device="cuda")
    a = N.from_depth(d, K, l, max_gap=0.5, image=True)
    b = N.from_depth(d, k_dev, step=2, max_gap=0.5)
    N.angular_error(a[0], a[1], b[0], b[1])
    acc.add(a[0], a[1], b[0], b[1])
    reconstruct.mesh(d, K, l, c, normals=a[0])                      # warm: code objects loaded
    acc = N.NormalErrorAccumulator(device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda").item()                     # the mode does catch a synchronisation
        a = N.from_depth(d, K, l, max_gap=0.5, image=True)
        b = N.from_depth(d, k_dev, step=2, max_gap=0.5)
        tables = N.angular_error(a[0], a[1], b[0], b[1])
        acc.add(a[0], a[1], b[0], b[1])
        m = reconstruct.mesh(d, K, l, c, normals=a[0])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    wa, wb = R.normals_vec(depth, K, labels, max_gap=0.5), R.normals_vec(depth, K, None, step=2, max_gap=0.5)
    assert R.same((a[0][0].cpu().numpy(), a[1][0].cpu().numpy(), a[2][0].cpu().numpy()), wa) and R.same((b[0][0].cpu().numpy(), b[1][0].cpu().numpy()), wb[:2])
    want = R.error_tables(wa[0], wa[1], wb[0], wb[1])
    assert np.array_equal(tables[0][0].cpu().numpy(), want[0]) and np.array_equal(acc.tables()[0], want[0]) and int(acc.tables()[2]) == int(want[2])
    nv = int(m.counts[0, 0])
    assert np.array_equal(_bits(m.normals[0, :nv].cpu().numpy()), _bits(wa[0][m.vertex_id[0].cpu().numpy() >= 0]))


def test_library_refuses_before_any_launch():
    """with real buffers: nothing is launched, the outputs keep their fill pattern"""
    from planerecnet_amd import _lib
    lib = _lib.lib
    H, W = 4, 6
    d = torch.full((H, W), 2.0).cuda()
    lab = torch.ones(H, W, dtype=torch.int32).cuda()
    k = torch.tensor([2.0, 0, 0.5, 0, 2.0, 0.5, 0, 0, 1.0], dtype=torch.float64).cuda()
    out_n = torch.full((H * W * 3,), -7, dtype=torch.int32).cuda()
    out_v = torch.full((H * W,), 7, dtype=torch.uint8).cuda()
    out_i = torch.full((H * W * 3,), 7, dtype=torch.uint8).cuda()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))
    inf = float("inf")

    def call(depth=d, labels=lab, kk=k, B=1, h=H, w=W, step=1, gap=0.05, flags=3, n=out_n, v=out_v, i=out_i):
        return lib.prn_normals(p(depth), p(labels), p(kk), B, h, w, step, 0.0, inf, gap, flags, p(n), p(v), p(i), st)

    for kw, msg in ((dict(h=4096, w=4096), b"2^24"), (dict(h=1 << 12, w=(1 << 12) + 1), b"2^24"), (dict(step=0), b"step"), (dict(step=-3), b"step"),
                    (dict(gap=-0.5), b"max_gap"), (dict(gap=float("nan")), b"max_gap"), (dict(gap=inf), b"max_gap"), (dict(B=0), b"B <= 65535"),
                    (dict(B=65536), b"B <= 65535"), (dict(h=0), b"positive"), (dict(w=-1), b"positive"), (dict(flags=8), b"flags"), (dict(depth=None), b"null"),
                    (dict(kk=None), b"null"), (dict(n=None), b"null"), (dict(v=None), b"null")):
        assert call(**kw) != 0 and msg in lib.prn_last_error(), (kw, lib.prn_last_error())
    hist = torch.full((R.BINS,), -7, dtype=torch.int64).cuda()
    within = torch.full((3,), -7, dtype=torch.int64).cuda()
    count = torch.full((1,), -7, dtype=torch.int64).cuda()
    a = torch.zeros(H * W, 3).cuda()
    va = torch.ones(H * W, dtype=torch.uint8).cuda()
    thr = (ctypes.c_double * 3)(0.1, 0.2, 0.3)

    def err(aa=a, v1=va, bb=a, v2=va, B=1, n=H * W, t=thr, T=3, h=hist, w=within, c=count):
        return lib.prn_normal_error(p(aa), p(v1), p(bb), p(v2), B, n, t, T, p(h), p(w), p(c), st)

    for kw, msg in ((dict(B=0), b"[1, 65535]"), (dict(B=65536), b"[1, 65535]"), (dict(n=0), b"2^31"), (dict(n=1 << 31), b"2^31"), (dict(T=9), b"T must"), (dict(T=-1), b"T must"),
                    (dict(t=None), b"thresholds"), (dict(w=None), b"thresholds"), (dict(aa=None), b"null"), (dict(v1=None), b"null"), (dict(bb=None), b"null"),
                    (dict(v2=None), b"null"), (dict(h=None), b"null"), (dict(c=None), b"null")):
        assert err(**kw) != 0 and msg in lib.prn_last_error(), (kw, lib.prn_last_error())
    torch.cuda.synchronize()
    assert int((out_n != -7).sum()) == 0 and int((out_v != 7).sum()) == 0 and int((out_i != 7).sum()) == 0
    assert all(int((t != -7).sum()) == 0 for t in (hist, within, count))
    assert call() == 0 and call(labels=None, i=None, flags=4) == 0 and err(T=0, t=None, w=None, h=hist.zero_(), c=count.zero_()) == 0
    torch.cuda.synchronize()
    assert out_v.tolist() == [1] * (H * W) and out_n.view(torch.float32).reshape(-1, 3).tolist() == [[0.0, 0.0, 1.0]] * (H * W)      # flags 4: the plane's side
    assert out_i.reshape(-1, 3).tolist() == [[0, 128, 128]] * (H * W)                                  # (written by the first call only)
    assert int(hist[0]) == H * W and int(count[0]) == H * W and int((within != -7).sum()) == 0


def test_mesh_integration():
    from planerecnet_amd import planes, reconstruct
    N = _n()
    H, W = 48, 64
    K = M.k_of(58.3, 57.9, 31.6, 23.7)
    rng = np.random.RandomState(11)
    results, owners = [], []
    for b, n in enumerate((3, 0, 2)):
        depth = M.scene(H, W, seed=20 + b, holes=0.0)[0]
        depth = np.where(np.isfinite(depth) & (depth > 0), depth, np.float32(3.0)).astype(np.float32)
        if b == 2:
            depth[rng.rand(H, W) < 0.05] = np.nan
        masks = np.zeros((n, H, W), bool)
        owner = np.zeros((H, W), np.int32)
        for i in range(n):
            y0, x0 = rng.randint(0, H // 2), rng.randint(0, W // 2)
            masks[i, y0:y0 + H // 2, x0:x0 + W // 2] = True
            owner[masks[i]] = i + 1
        results.append({"pred_depth": _t(depth)[None, None], "pred_masks": _t(masks) if n else None})
        owners.append(owner)
    d = torch.cat([r["pred_depth"] for r in results])
    n, ok, _ = N.from_depth(d, K, _t(np.stack(owners)), step=2, max_gap=0.1)
    m = reconstruct.mesh(d, K, _t(np.stack(owners)), normals=n)
    assert m.normals.shape == (3, H * W, 3) and m.normals.is_cuda
    for b, got in enumerate(m.cpu()):
        want = R.normals_vec(d[b, 0].cpu().numpy(), K, owners[b], step=2, max_gap=0.1)
        vid = m.vertex_id[b].cpu().numpy()
        assert got["normals"].shape == got["vertices"].shape and np.array_equal(_bits(got["normals"]), _bits(want[0][vid >= 0])), b
    assert "normals" not in reconstruct.mesh(d, K).cpu()[0]
    plain = reconstruct.reconstruct_results(results, K)
    for kw in ({}, {"step": 2, "max_gap": 0.1}):
        r = reconstruct.reconstruct_results(results, K, normals=kw)
        assert torch.equal(r.counts, plain.counts) and torch.equal(r.vertex_id, plain.vertex_id)
        for b, got in enumerate(r.cpu()):
            want = R.normals_vec(d[b, 0].cpu().numpy(), K, owners[b], **kw)
            assert np.array_equal(_bits(got["normals"]), _bits(want[0][r.vertex_id[b].cpu().numpy() >= 0])), (b, kw)
    planar = planes.planar_depth(results, K, depth_range=(0.0, 10.0))
    r = reconstruct.reconstruct_results(planar, K, normals={"max_gap": 0.1})
    pd = planar[0]["pred_plane_depth"].squeeze().cpu().numpy()
    want = R.normals_vec(pd, K, owners[0], max_gap=0.1)
    assert np.array_equal(_bits(r.cpu()[0]["normals"]), _bits(want[0][r.vertex_id[0].cpu().numpy() >= 0]))


class _SceneDataset:
    """frames with the contract of SyntheticPlaneDataset whose depth is a scene: (image [3,H,W], instances, depth [1,H,W])"""

    def __init__(self, n, hw=(48, 64)):
        self.n, self.hw = n, hw

    def __len__(self):
        return self.n

    def pull_item(self, i):
        H, W = self.hw
        depth, labels, _, K = M.scene(H, W, seed=40 + i, holes=0.0)
        depth = np.where(np.isfinite(depth) & (depth > 0), depth, np.float32(3.0)).astype(np.float32)
        masks = np.stack([labels == k for k in (1, 2)]).astype(np.uint8)
        boxes = np.array([[0, 0, W, H]] * 2, np.float64)
        image = torch.zeros(3, H, W)
        image[0, 0, 0] = float(i + 1)
        inst = {"masks": torch.from_numpy(masks), "boxes": torch.from_numpy(boxes), "classes": torch.zeros(2, dtype=torch.int64), "k_matrix": torch.from_numpy(K)}
        return image, inst, torch.from_numpy(depth)[None]


class _StubNet(torch.nn.Module):
    """returns a prepared eval-mode result for the frame whose first pixel the image carries"""

    def __init__(self, results):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.results = results

    def forward(self, x):
        return [self.results[float(x[0, 0, 0, 0].item())]]


def test_evaluate_normal_metrics():
    import eval as ev
    from planerecnet_amd import metrics
    dataset = _SceneDataset(3)
    results, pooled = {}, None
    for i in range(3):
        image, inst, depth = dataset.pull_item(i)
        H, W = depth.shape[-2:]
        u = np.mgrid[:H, :W][1]
        pred = (depth[0].numpy() * (1.03 + 0.02 * np.sin(u / 5.0 + i))).astype(np.float32)      # another scale (no effect) and a ripple (the error)
        dm = (inst["masks"] != 0).cuda()
        results[float(image[0, 0, 0])] = {"pred_masks": dm, "pred_boxes": metrics.mask_boxes(dm).cpu(), "pred_classes": torch.zeros(2).cuda(),
                                          "pred_scores": torch.linspace(0.9, 0.5, 2).cuda(), "pred_depth": _t(pred)[None]}
        K = inst["k_matrix"].numpy()
        a, b = R.normals_vec(pred, K), R.normals_vec(depth[0].numpy(), K)
        tables = R.error_tables(a[0], a[1], b[0], b[1])
        pooled = tables if pooled is None else tuple(x + y for x, y in zip(pooled, tables))
    net = _StubNet(results).cuda()
    ev.parse_args(["--no_bar"])
    with torch.no_grad():
        random.seed(0)
        buf = io.StringIO()
        with redirect_stdout(buf):
            table, got = ev.evaluate(net, dataset, eval_nums=3, normal_metrics=True)
        random.seed(0)
        plain_buf = io.StringIO()
        with redirect_stdout(plain_buf):
            plain_table, plain = ev.evaluate(net, dataset, eval_nums=3)
    keys = ["normal_mean", "normal_median", "normal_rmse", "normal_11.25", "normal_22.5", "normal_30", "normal_pixels"]
    assert list(plain) == list(metrics.depth_metrics) and plain_table == table and list(got) == list(metrics.depth_metrics) + keys
    assert all(got[k] == plain[k] or (got[k] != got[k] and plain[k] != plain[k]) for k in plain)
    hist, within, count = pooled
    n = int(count)
    theta = np.degrees(2.0 * np.arcsin(np.minimum(1.0, (np.arange(R.BINS) + 0.5) * 2.0 / R.BINS / 2.0)))
    assert got["normal_pixels"] == n > 3 * 48 * 64 // 2
    assert got["normal_mean"] == pytest.approx(float((hist * theta).sum() / n), rel=1e-12) and got["normal_rmse"] == pytest.approx(math.sqrt((hist * theta ** 2).sum() / n), rel=1e-12)
    assert got["normal_median"] == theta[np.flatnonzero(np.cumsum(hist) >= (n + 1) // 2)[0]]
    assert [got["normal_11.25"], got["normal_22.5"], got["normal_30"]] == [int(w) / n for w in within] and 0.0 < got["normal_11.25"] <= got["normal_30"] <= 1.0
    assert 0.0 < got["normal_mean"] < 45.0
    text = buf.getvalue().splitlines()
    at = text.index("Normal Metrics:")
    assert text[at + 1] == "mean: %.5f, median: %.5f, rmse: %.5f, 11.25: %.5f, 22.5: %.5f, 30: %.5f" % tuple(got[k] for k in keys[:6])
    assert "Normal Metrics:" not in plain_buf.getvalue()
    extra = [ln for ln in text if ln not in plain_buf.getvalue().splitlines()]
    assert len(extra) == 2                                           # the flag adds its two lines and changes none


def test_simple_inference_writes_the_normal_picture_and_ply_normals(tmp_path):
    import simple_inference as si
    from PIL import Image
    from planerecnet_amd import reconstruct
    H, W = 48, 64
    depth, _, colors, K = M.scene(H, W, seed=9, holes=0.02)
    masks = np.zeros((2, H, W), bool)
    masks[0, 5:30, 4:40] = True
    masks[1, 20:44, 30:60] = True
    owner = np.zeros((H, W), np.int32)
    owner[masks[0]] = 1
    owner[masks[1]] = 2                                              # painted in index order: the last wins
    result = {"pred_depth": _t(depth)[None, None], "pred_masks": _t(masks)}
    old = getattr(si, "args", None)
    try:
        si.parse_args(["--image", "frame.png", "--normals", "--normals_step", "2", "--normals_gap", "0.5", "--intrinsics", "1,1,1,1", "--ply", "--ply_normals"])
        path = str(tmp_path / "frame_normals.png")
        n, ok = si.write_normals(path, result, K)
        si.write_mesh(str(tmp_path / "frame_mesh.ply"), result, K, colors)
    finally:
        si.args = old
    want = R.normals_vec(depth, K, owner, step=2, max_gap=0.5)
    assert want[1].sum() > 1000 and R.same((n.cpu().numpy(), ok.cpu().numpy()), want[:2])
    shown = np.asarray(Image.open(path))
    assert shown.shape == (H, W, 3) and np.array_equal(shown[:, :, ::-1], want[2])               # the file is RGB = (x, y, z)
    ply = reconstruct.read_ply(str(tmp_path / "frame_mesh.ply"))
    plain = M.mesh_vec(depth, K, owner, colors)
    assert np.array_equal(_bits(ply["vertices"]), _bits(plain["vertices"])) and np.array_equal(ply["faces"], plain["faces"])
    assert np.array_equal(_bits(ply["normals"]), _bits(want[0][plain["vertex_id"] >= 0]))
