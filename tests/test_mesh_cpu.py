"""CPU: the mesh rules of DESIGN.md section 22 -- the restatement's two forms against each other, planerecnet_amd.reconstruct's numpy path
against the restatement (bit for bit), hand-made cases with known answers, the PLY writer and reader, host refusals, the CLI flags."""
import math
import os

import numpy as np
import pytest
import torch

import mesh_restate as R

K22 = R.k_of(2.0, 2.0, 0.5, 0.5)


def _rc():
    import __graft_entry__ as g
    g.build()
    from planerecnet_amd import reconstruct
    return reconstruct


def _mesh(depth, K=K22, labels=None, colors=None, **kw):
    """reconstruct.mesh on CPU tensors of one image -> restatement-style dict"""
    m = _rc().mesh(torch.from_numpy(np.asarray(depth, np.float32)), K, None if labels is None else torch.from_numpy(np.asarray(labels, np.int32)),
                   None if colors is None else torch.from_numpy(np.asarray(colors, np.uint8)), **kw)
    return R.from_mesh(m)[0]


def _faces(depth, **kw):
    return [tuple(int(i) for i in t) for t in _mesh(depth, **kw)["faces"]]


CASES = [dict(), dict(relative=False, max_gap=0.02), dict(same_label=False), dict(planar_only=True), dict(depth_range=(1.5, 3.0)),
         dict(faces=False), dict(max_gap=0.0), dict(planar_only=True, same_label=False, relative=False, max_gap=1.0, depth_range=(0.5, 100.0))]


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (6, 1), (2, 2), (5, 9), (13, 8)])
def test_restatement_forms_agree(shape):
    for seed, kw in enumerate(CASES):
        depth, labels, colors, K = R.scene(*shape, seed=seed, holes=0.15)
        assert R.same(R.mesh_loop(depth, K, labels, colors, **kw), R.mesh_vec(depth, K, labels, colors, **kw)), (shape, kw)
    depth, labels, _, K = R.scene(*shape, seed=9, holes=0.1)
    assert R.same(R.mesh_loop(depth, K), R.mesh_vec(depth, K))                       # no labels, no colours


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (6, 1), (2, 2), (13, 8), (37, 65), (480, 640)])
def test_numpy_path_against_the_restatement(shape):
    for seed, kw in enumerate(CASES if shape != (480, 640) else CASES[:2]):
        depth, labels, colors, K = R.scene(*shape, seed=seed, holes=0.02)
        got, want = _mesh(depth, K, labels, colors, **kw), R.mesh_vec(depth, K, labels, colors, **kw)
        assert R.same(got, want), (shape, kw)
        assert shape[0] < 13 or (want["counts"][0] > 0 and (want["counts"][1] > 0 or kw.get("faces") is False or kw.get("max_gap") == 0.0)), (shape, kw)
    depth, labels, _, K = R.scene(*shape, seed=3)
    assert R.same(_mesh(depth, K), R.mesh_vec(depth, K))


def test_batch_and_input_forms():
    rc = _rc()
    scenes = [R.scene(9, 11, seed=s, holes=0.1) for s in range(3)]
    scenes[1][0][:] = np.nan                                                          # one image all invalid
    Ks = np.stack([s[3] * (1.0 + 0.1 * i) for i, s in enumerate(scenes)])
    d = torch.from_numpy(np.stack([s[0] for s in scenes]))[:, None]
    lab = torch.from_numpy(np.stack([s[1] for s in scenes]))
    col = torch.from_numpy(np.stack([s[2] for s in scenes]))
    m = rc.mesh(d, Ks, lab, col)
    assert m.vertices.shape == (3, 99, 3) and m.faces.shape == (3, 160, 3) and m.labels.shape == (3, 99) and m.colors.shape == (3, 99, 3)
    assert m.counts.dtype == torch.int32 and m.vertex_id.shape == (3, 9, 11) and m.counts[1].tolist() == [0, 0]
    for b, got in enumerate(R.from_mesh(m)):
        assert R.same(got, R.mesh_vec(scenes[b][0], Ks[b], scenes[b][1], scenes[b][2]))
    one = rc.mesh(d[0], torch.from_numpy(Ks[0]), lab[0], col[0])                      # [1,H,W] depth, [H,W] labels, tensor K
    assert R.same(R.from_mesh(one)[0], R.mesh_vec(scenes[0][0], Ks[0], scenes[0][1], scenes[0][2]))
    pc = rc.point_cloud(d, Ks, lab, col, planar_only=True)
    assert pc.faces is None and pc.counts[:, 1].tolist() == [0, 0, 0]
    assert R.same(R.from_mesh(pc)[2], R.mesh_vec(scenes[2][0], Ks[2], scenes[2][1], scenes[2][2], planar_only=True, faces=False))


def test_two_by_two_and_one_invalid_corner():
    flat = np.full((2, 2), 2.0, np.float32)
    m = _mesh(flat)
    assert m["vertex_id"].tolist() == [[0, 1], [2, 3]]                                # row-major ids: a = 0, c = 1, b = 2, d = 3 ...
    assert _faces(flat) == [(0, 2, 1), (1, 2, 3)]                                     # ... so t0 = (a,b,c) = (0,2,1), t1 = (c,b,d) = (1,2,3)
    assert np.array_equal(m["vertices"], np.array([[-0.5, -0.5, 2], [0.5, -0.5, 2], [-0.5, 0.5, 2], [0.5, 0.5, 2]], np.float32))
    for hole, want in (((0, 0), [(0, 1, 2)]), ((1, 1), [(0, 2, 1)]), ((0, 1), []), ((1, 0), [])):
        z = flat.copy()
        z[hole] = np.nan
        assert _faces(z) == want, hole


def test_two_by_two_in_corner_numbers():
    """A 2 x 2 image gives exactly [(0,1,2), (2,1,3)] with its corners numbered a, b, c, d = 0, 1, 2, 3 (t0 = (a,b,c), t1 = (c,b,d)).  In
    vertex ids -- row-major, so b = (1,0) comes after c = (0,1) -- the same two faces read (0,2,1), (1,2,3): the test above."""
    m = _mesh(np.full((2, 2), 1.0, np.float32))
    vid = m["vertex_id"]
    corner = {int(vid[0, 0]): 0, int(vid[1, 0]): 1, int(vid[0, 1]): 2, int(vid[1, 1]): 3}
    assert [tuple(corner[i] for i in t) for t in m["faces"].tolist()] == [(0, 1, 2), (2, 1, 3)]


def test_gap_rule_on_the_boundary():
    up = np.nextafter(np.float32(2.5), np.float32(3.0))
    for relative, gap in ((True, 0.25), (False, 0.5)):
        z = np.array([[2.0, 2.0], [2.5, 2.0]], np.float32)                            # b = 2.5: in both triangles
        assert len(_faces(z, max_gap=gap, relative=relative)) == 2                    # 0.5 <= 0.5
        z[1, 0] = up
        assert len(_faces(z, max_gap=gap, relative=relative)) == 0
        z = np.array([[2.0, 2.0], [2.0, up]], np.float32)                             # d only: t0 stays
        assert _faces(z, max_gap=gap, relative=relative) == [(0, 2, 1)]
    assert len(_faces(np.array([[2.0, 2.0], [2.5, 2.0]], np.float32), max_gap=0.0)) == 0
    assert len(_faces(np.full((2, 2), 3.0, np.float32), max_gap=0.0)) == 2


def test_label_seam_planar_only_and_depth_values():
    z = np.full((3, 4), 2.0, np.float32)
    lab = np.array([[1, 1, 2, 2]] * 3, np.int32)
    got = _mesh(z, labels=lab)
    assert got["counts"] == (12, 8)                                                   # the quads of column 1 straddle the seam: 4 triangles gone
    vid = got["vertex_id"]
    assert all(len({int(lab.ravel()[i]) for i in t}) == 1 for t in got["faces"])
    assert not any({int(vid[0, 1]), int(vid[0, 2])} <= set(t.tolist()) for t in got["faces"])
    assert _mesh(z, labels=lab, same_label=False)["counts"] == (12, 12)
    lab0 = lab.copy()
    lab0[:, 0] = 0
    assert _mesh(z, labels=lab0, planar_only=True)["counts"] == (9, 4) and _mesh(z, labels=lab0)["counts"] == (12, 4)
    assert _mesh(z, planar_only=True)["counts"] == (0, 0)                             # no labels: all 0
    bad = np.array([[np.nan, np.inf, -np.inf, 0.0, -1.0, 1.0, 5.0]], np.float32)
    assert _mesh(bad)["vertex_id"].tolist() == [[-1, -1, -1, -1, -1, 0, 1]]
    assert _mesh(bad, depth_range=(1.0, 5.0))["counts"] == (0, 0)                     # both ends open
    assert _mesh(bad, depth_range=(-2.0, 2.0))["vertex_id"].tolist() == [[-1, -1, -1, 0, 1, 2, -1]]


def test_degenerate_sizes():
    for shape in ((1, 5), (5, 1), (1, 1)):
        m = _mesh(np.full(shape, 1.5, np.float32))
        assert m["counts"] == (shape[0] * shape[1], 0) and m["faces"].shape == (0, 3)
    m = _mesh(np.full((4, 5), np.nan, np.float32), colors=np.zeros((4, 5, 3), np.uint8))
    assert m["counts"] == (0, 0) and m["vertices"].shape == (0, 3) and m["colors"].shape == (0, 3) and (m["vertex_id"] == -1).all()


def test_triangles_face_the_camera_and_ids_are_the_running_count():
    depth, labels, colors, K = R.scene(48, 64, seed=4, holes=0.03)
    m = _mesh(depth, K, labels, colors, same_label=False, max_gap=10.0)
    nv, nf = m["counts"]
    assert nf > 1000 and m["faces"].min() >= 0 and m["faces"].max() < nv
    p = m["vertices"].astype(np.float64)[m["faces"]]                                  # [F,3,3]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert ((n * p.mean(1)).sum(1) < 0).all()
    ok = m["vertex_id"] >= 0
    assert np.array_equal(m["vertex_id"][ok], np.arange(nv)) and np.array_equal(np.cumsum(ok.ravel())[ok.ravel()] - 1, m["vertex_id"][ok])
    assert np.array_equal(m["labels"], labels[ok]) and np.array_equal(m["colors"], colors[ok]) and np.array_equal(m["vertices"][:, 2], depth[ok])


# ---- PLY ----

def _small():
    depth, labels, colors, K = R.scene(7, 9, seed=2, holes=0.1)
    depth[0, 0], depth[0, 1] = np.float32(1e-30), np.float32(3.4e38)                  # extreme values must read back exactly too
    d = _mesh(depth, K, labels, colors, same_label=False, max_gap=1e30)
    return {k: d[k] for k in ("vertices", "faces", "labels", "colors")}


def test_ply_header_is_byte_for_byte(tmp_path):
    rc, d = _rc(), _small()
    nv, nf = d["vertices"].shape[0], d["faces"].shape[0]
    p = str(tmp_path / "a.ply")
    rc.write_ply(p, d, binary=True, comment=["made by a test", "second line"])
    want = ("ply\nformat binary_little_endian 1.0\ncomment made by a test\ncomment second line\nelement vertex %d\nproperty float x\nproperty float y\n"
            "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty int label\nelement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (nv, nf)).encode()
    raw = open(p, "rb").read()
    assert raw.startswith(want) and len(raw) == len(want) + nv * 19 + nf * 13
    assert raw[len(want):len(want) + 12] == d["vertices"][0].astype("<f4").tobytes() and raw[-13:] == b"\x03" + d["faces"][-1].astype("<i4").tobytes()
    rc.write_ply(p, {"vertices": d["vertices"], "labels": d["labels"]}, binary=False)
    want = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty int label\nend_header\n" % nv).encode()
    assert open(p, "rb").read().startswith(want)


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("drop", [(), ("faces",), ("colors",), ("faces", "colors")])
def test_ply_round_trip_is_exact(tmp_path, binary, drop):
    rc, d = _rc(), _small()
    for k in drop:
        d[k] = None
    p = str(tmp_path / "m.ply")
    rc.write_ply(p, d, binary=binary, comment="c" if binary else None)
    back = rc.read_ply(p)
    assert back["comments"] == (["c"] if binary else [])
    for k in ("vertices", "faces", "labels", "colors"):
        if d[k] is None:
            assert back[k] is None
        else:
            assert back[k].dtype == d[k].dtype and back[k].shape == d[k].shape and back[k].tobytes() == d[k].tobytes(), k
    empty = {"vertices": np.zeros((0, 3), np.float32), "labels": np.zeros(0, np.int32), "colors": None, "faces": np.zeros((0, 3), np.int32)}
    rc.write_ply(p, empty, binary=binary)
    back = rc.read_ply(p)
    assert back["vertices"].shape == (0, 3) and back["faces"].shape == (0, 3) and back["colors"] is None


def test_read_ply_refuses_what_write_ply_did_not_make(tmp_path):
    rc, d = _rc(), _small()
    p, q = str(tmp_path / "m.ply"), str(tmp_path / "bad.ply")
    for binary in (True, False):
        rc.write_ply(p, d, binary=binary)
        raw = open(p, "rb").read()
        variants = [raw[:-1], raw[:-7], raw + b"\n", raw[:len(raw) // 2], raw[:20],
                    raw.replace(b"property float x", b"property double x"), raw.replace(b"ply\n", b"ply\r\n", 1),
                    raw.replace(b"property int label\n", b"property int label\nproperty float nx\n"),
                    raw.replace(b"format ", b"format  ", 1), raw.replace(b"vertex_indices", b"vertex_index")]
        for i, v in enumerate(variants):
            open(q, "wb").write(v)
            with pytest.raises(ValueError):
                rc.read_ply(q)
    open(q, "wb").write(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nproperty int label\nend_header\n")
    with pytest.raises(ValueError):
        rc.read_ply(q)
    with pytest.raises(ValueError):
        rc.write_ply(q, d, comment="two\nlines")


# ---- refusals ----

def test_host_refusals():
    rc = _rc()
    z = torch.ones(4, 5)
    K = K22
    for bad in (z.double(), z.half(), torch.ones(5), torch.ones(2, 4, 5), torch.ones(2, 2, 4, 5), z.numpy(), torch.ones(0, 5), None):
        with pytest.raises(RuntimeError):
            rc.mesh(bad, K)
    for lab in (torch.zeros(4, 5, dtype=torch.int64), torch.zeros(5, 4, dtype=torch.int32), torch.zeros(2, 4, 5, dtype=torch.int32), np.zeros((4, 5), np.int32),
                torch.zeros(4, 5, dtype=torch.int32, device="meta")):
        with pytest.raises(RuntimeError):
            rc.mesh(z, K, labels=lab)
    for col in (torch.zeros(4, 5, 3), torch.zeros(4, 5, 4, dtype=torch.uint8), torch.zeros(3, 4, 5, dtype=torch.uint8),
                torch.zeros(4, 5, 3, dtype=torch.uint8, device="meta")):
        with pytest.raises(RuntimeError):
            rc.mesh(z, K, colors=col)
    for k in (np.eye(4), np.zeros((2, 3, 3)), np.zeros(9)):
        with pytest.raises(RuntimeError):
            rc.mesh(z, k)
    for gap in (-1e-9, float("nan"), float("inf"), -float("inf"), 1e39, "0.1", None, True):
        with pytest.raises(ValueError):
            rc.mesh(z, K, max_gap=gap)
    for rng in ((float("nan"), 1.0), (0.0,), 3.0, (0.0, "x")):
        with pytest.raises(ValueError):
            rc.mesh(z, K, depth_range=rng)
    big = torch.zeros(1).expand(4096, 4096)                                           # 2^24 pixels by shape alone: nothing is allocated
    with pytest.raises(RuntimeError, match="2\\^24"):
        rc.mesh(big, K)
    with pytest.raises(RuntimeError, match="2\\^24"):
        rc.mesh(torch.zeros(1).expand(3, 1, 1 << 12, 1 << 13), K)
    assert rc.mesh(z, K, max_gap=0).counts.tolist() == [[20, 24]] and rc.mesh(z, K, max_gap=np.float32(0.5)).counts.tolist() == [[20, 24]]


def test_library_refuses_on_the_host():
    """no GPU: every refusal comes before any launch (rc != 0 and a message)"""
    import ctypes
    from planerecnet_amd import _lib
    _rc()
    lib = _lib.lib
    p = ctypes.c_void_p(4096)                                                          # (never dereferenced)
    inf = float("inf")

    def call(H=4, W=5, B=1, gap=0.05, flags=11, colors=None, vcolors=None, ws=p, depth=p):
        return lib.prn_mesh(depth, p, colors, p, B, H, W, 0.0, inf, gap, flags, ws, p, p, vcolors, p, p, p, None)
    for kw, word in ((dict(H=4096, W=4096), "2^24"), (dict(gap=-1.0), "max_gap"), (dict(gap=float("nan")), "max_gap"), (dict(gap=inf), "max_gap"),
                     (dict(B=0), "B"), (dict(B=65536), "B"), (dict(H=0), "positive"), (dict(flags=16), "flags"), (dict(colors=p), "together"),
                     (dict(vcolors=p), "together"), (dict(ws=ctypes.c_void_p(4100)), "aligned"), (dict(depth=None), "null")):
        assert call(**kw) != 0 and word in lib.prn_last_error().decode(), kw
    assert lib.prn_mesh_ws_bytes(1, 4096, 4096) == -1 and lib.prn_mesh_ws_bytes(0, 4, 4) == -1
    px = lib.prn_mesh_block_pixels()
    assert px > 0 and px % 64 == 0 and lib.prn_mesh_scan_chunk() > 0
    assert lib.prn_mesh_ws_bytes(3, 1, px + 1) == 3 * 2 * 8 and lib.prn_mesh_ws_bytes(1, 1, px) == 8


# ---- command line ----

def test_parse_args_for_the_ply_flags(capsys):
    import simple_inference as si
    a = si.parse_args(["--ibims1_pd", "in:out"])
    assert a.ply is False and a.ply_gap == 0.05 and a.ply_absolute is False and a.ply_planar_only is False and a.intrinsics is None
    a = si.parse_args(["--ibims1", "in:out", "--ply", "--ply_gap", "0.1", "--ply_absolute", "--ply_planar_only"])
    assert a.ply and a.ply_gap == 0.1 and a.ply_absolute and a.ply_planar_only
    assert si.mesh_options() == {"max_gap": 0.1, "relative": False, "planar_only": True}
    a = si.parse_args(["--image", "a.png", "--ply", "--intrinsics", "518.9,519.5,325.6,253.7"])
    assert a.intrinsics == (518.9, 519.5, 325.6, 253.7)
    for argv in (["--image", "a.png", "--ply"], ["--image", "a.png", "--ply", "--intrinsics", "1,2,3"], ["--image", "a.png", "--ply", "--intrinsics", "a,b,c,d"],
                 ["--ibims1", "i:o", "--ply", "--ply_gap", "-1"], ["--ibims1", "i:o", "--ply", "--ply_gap", "nan"], ["--images", "i:o", "--ply"]):
        with pytest.raises(SystemExit):
            si.parse_args(argv)
        assert capsys.readouterr().err
    si.parse_args([])


def test_reconstruct_results_on_cpu_tensors():
    """the convenience layer needs no device: depth / masks / frames picked as documented"""
    rc = _rc()
    depth, _, colors, K = R.scene(9, 12, seed=6, holes=0.05)
    masks = np.zeros((3, 9, 12), bool)
    masks[0, :5], masks[1, 3:, :7], masks[2, 6:, 5:] = True, True, True
    owner = np.zeros((9, 12), np.int32)
    for i in range(3):
        owner[masks[i]] = i + 1                                                       # painted in index order: the last wins
    plane = depth + np.float32(0.25)
    r = {"pred_depth": torch.from_numpy(depth)[None, None], "pred_masks": torch.from_numpy(masks), "pred_plane_depth": torch.from_numpy(plane)[None, None]}
    r2 = {"pred_depth": torch.from_numpy(depth)[None], "pred_masks": None}
    m = rc.reconstruct_results([r, r2], K, frames=[colors, colors], planar_only=False)
    a, b = R.from_mesh(m)
    assert R.same(a, R.mesh_vec(plane, K, owner, colors)) and R.same(b, R.mesh_vec(depth, K, None, colors))
    m = rc.reconstruct_results([r2], K)
    assert m.colors is None and R.same(R.from_mesh(m)[0], R.mesh_vec(depth, K))
    r3 = dict(r, pred_plane_masks=torch.from_numpy(masks[:1]))
    assert R.same(R.from_mesh(rc.reconstruct_results([r3], K))[0], R.mesh_vec(plane, K, masks[0].astype(np.int32)))
