"""A plain-numpy restatement of the mesh rules, written from the definitions and sharing no code with
planerecnet_amd/reconstruct.py: `mesh_loop` walks pixels and quads one by one (tiny images), `mesh_vec` is vectorised (480 x 640).
Both take one image and return a dict: vertices [Nv,3] float32, labels [Nv] int32, colors [Nv,3] uint8 or None, faces [Nf,3] int32
(None with faces=False), vertex_id [H,W] int32, counts (Nv, Nf).  Helpers make the test scenes."""
import numpy as np

F32 = np.float32


def _k4(K):
    K = np.asarray(K, dtype=np.float64)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def mesh_loop(depth, K, labels=None, colors=None, depth_range=(0.0, np.inf), max_gap=0.05, relative=True, same_label=True, planar_only=False,
              faces=True):
    depth = np.asarray(depth, dtype=F32)
    H, W = depth.shape
    labels = np.zeros((H, W), np.int32) if labels is None else np.asarray(labels, dtype=np.int32)
    fx, fy, cx, cy = _k4(K)
    lo, hi, gap = F32(depth_range[0]), F32(depth_range[1]), F32(max_gap)

    def valid(v, u):
        z = depth[v, u]
        return bool(np.isfinite(z) and lo < z and z < hi and (not planar_only or labels[v, u] > 0))

    vid = np.full((H, W), -1, np.int32)
    verts, vlab, vcol = [], [], []
    with np.errstate(all="ignore"):
        for v in range(H):
            for u in range(W):
                if not valid(v, u):
                    continue
                vid[v, u] = len(verts)
                z = depth[v, u]
                X = (np.float64(u) - cx) * np.float64(z) / fx
                Y = (np.float64(v) - cy) * np.float64(z) / fy
                verts.append((F32(X), F32(Y), z))
                vlab.append(labels[v, u])
                if colors is not None:
                    vcol.append(tuple(colors[v, u]))
        tris = []
        if faces:
            for v in range(H - 1):
                for u in range(W - 1):
                    a, b, c, d = (v, u), (v + 1, u), (v, u + 1), (v + 1, u + 1)
                    for t in ((a, b, c), (c, b, d)):
                        if not all(valid(*q) for q in t):
                            continue
                        if same_label and not (labels[t[0]] == labels[t[1]] == labels[t[2]]):
                            continue
                        zs = [depth[q] for q in t]
                        zmax, zmin = max(zs), min(zs)
                        spread = F32(zmax - zmin)
                        bound = F32(gap * zmin) if relative else gap
                        if spread <= bound:
                            tris.append([vid[q] for q in t])
    return {"vertices": np.array(verts, dtype=F32).reshape(-1, 3), "labels": np.array(vlab, dtype=np.int32).reshape(-1),
            "colors": None if colors is None else np.array(vcol, dtype=np.uint8).reshape(-1, 3),
            "faces": np.array(tris, dtype=np.int32).reshape(-1, 3) if faces else None, "vertex_id": vid, "counts": (len(verts), len(tris))}


def mesh_vec(depth, K, labels=None, colors=None, depth_range=(0.0, np.inf), max_gap=0.05, relative=True, same_label=True, planar_only=False,
             faces=True):
    depth = np.asarray(depth, dtype=F32)
    H, W = depth.shape
    labels = np.zeros((H, W), np.int32) if labels is None else np.asarray(labels, dtype=np.int32)
    fx, fy, cx, cy = _k4(K)
    lo, hi, gap = F32(depth_range[0]), F32(depth_range[1]), F32(max_gap)
    with np.errstate(all="ignore"):
        ok = np.isfinite(depth) & (lo < depth) & (depth < hi)
        if planar_only:
            ok = ok & (labels > 0)
        order = np.flatnonzero(ok.ravel())                           # row-major positions of the vertices
        vid = np.full(H * W, -1, np.int32)
        vid[order] = np.arange(order.size, dtype=np.int32)
        vid = vid.reshape(H, W)
        vv, uu = np.divmod(order, W)
        z64 = depth.ravel()[order].astype(np.float64)
        verts = np.empty((order.size, 3), F32)
        verts[:, 0] = ((uu.astype(np.float64) - cx) * z64 / fx).astype(F32)
        verts[:, 1] = ((vv.astype(np.float64) - cy) * z64 / fy).astype(F32)
        verts[:, 2] = depth.ravel()[order]
        tris = None
        if faces:
            qv, qu = np.meshgrid(np.arange(H - 1), np.arange(W - 1), indexing="ij")
            qv, qu = qv.ravel(), qu.ravel()
            a, b, c, d = (qv, qu), (qv + 1, qu), (qv, qu + 1), (qv + 1, qu + 1)
            out = np.full((qv.size, 2, 3), -1, np.int32)
            emit = np.zeros((qv.size, 2), bool)
            for j, t in enumerate(((a, b, c), (c, b, d))):
                e = ok[t[0]] & ok[t[1]] & ok[t[2]]
                if same_label:
                    e &= (labels[t[0]] == labels[t[1]]) & (labels[t[0]] == labels[t[2]])
                zs = np.stack([depth[q] for q in t])
                zmin = zs.min(0)
                spread = (zs.max(0) - zmin).astype(F32)
                bound = (gap * zmin).astype(F32) if relative else gap
                emit[:, j] = e & (spread <= bound)
                for i, q in enumerate(t):
                    out[:, j, i] = vid[q]
            tris = out[emit]
    nf = 0 if tris is None else tris.shape[0]
    return {"vertices": verts, "labels": labels.ravel()[order], "colors": None if colors is None else np.asarray(colors).reshape(-1, 3)[order],
            "faces": tris, "vertex_id": vid, "counts": (order.size, nf)}


def same(x, y):
    """two restatement-style dicts agree bit for bit (floats compared as bits: -0.0 and NaN payloads count)"""
    for key in ("vertices", "labels", "colors", "faces", "vertex_id"):
        p, q = x[key], y[key]
        if (p is None) != (q is None):
            return False
        if p is None:
            continue
        p, q = np.ascontiguousarray(p), np.ascontiguousarray(q)
        if p.shape != q.shape or p.dtype != q.dtype or p.tobytes() != q.tobytes():
            return False
    return tuple(int(v) for v in x["counts"]) == tuple(int(v) for v in y["counts"])


def from_mesh(m):
    """planerecnet_amd.reconstruct.Mesh -> one restatement-style dict per image"""
    imgs = m.cpu()
    counts, vid = m.counts.cpu().numpy(), m.vertex_id.cpu().numpy()
    for b, d in enumerate(imgs):
        d["vertex_id"] = vid[b]
        d["counts"] = (int(counts[b, 0]), int(counts[b, 1]))
    return imgs


def k_of(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=np.float64)


def scene(H, W, seed=0, holes=0.01):
    """a floor, a wall and a box with `holes` of the pixels made NaN / inf / 0 / negative -> (depth float32, labels int32, colors uint8, K)"""
    rng = np.random.RandomState(seed)
    K = k_of(0.9 * W + 0.37, 0.9 * W - 0.21, 0.5 * W - 0.4, 0.5 * H + 0.3)
    v, u = np.mgrid[:H, :W].astype(np.float64)
    ry = (v - K[1, 2]) / K[1, 1]
    rx = (u - K[0, 2]) / K[0, 0]
    with np.errstate(all="ignore"):
        floor = np.where(ry > 1e-3, 1.2 / ry, np.inf)              # the plane Y = 1.2
        wall = 4.0 / (1.0 + 0.3 * rx)                              # a slanted wall
    depth = np.minimum(floor, wall)
    labels = np.where(floor < wall, 1, 2).astype(np.int32)
    box = (np.abs(rx + 0.1) < 0.18) & (np.abs(ry - 0.1) < 0.15)
    depth = np.where(box, 2.0 + 0.1 * rx, depth)
    labels = np.where(box, 3, labels).astype(np.int32)
    labels[: max(1, H // 10)] = 0                                   # a band no plane owns
    depth = (depth + 1e-3 * rng.randn(H, W)).astype(F32)
    bad = rng.rand(H, W) < holes
    depth[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -1.5], dtype=F32), size=int(bad.sum()))
    colors = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    return depth, labels, colors, K
