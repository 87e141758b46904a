"""A plain-numpy restatement of the normal rules, written from the definitions and sharing no code with
planerecnet_amd/normals.py: `normals_loop` walks the pixels one by one (tiny images), `normals_vec` gathers the neighbours through index
arrays (480 x 640).  Both take one image and return (normals [H,W,3] float32, valid [H,W] bool, image [H,W,3] uint8).  `error_tables`
restates the angular-error tables with np.bincount, `exact_angles` gives the angles the histogram approximates."""
import numpy as np

F32, F64 = np.float32, np.float64
BINS = 4096


def _k4(K):
    K = np.asarray(K, dtype=F64)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def _byte(c):
    return np.uint8(np.rint((F64(c) * F64(0.5) + F64(0.5)) * F64(255.0)))


def normals_loop(depth, K, labels=None, step=1, max_gap=0.05, relative=True, same_label=True, depth_range=(0.0, np.inf), sign="camera"):
    depth = np.asarray(depth, dtype=F32)
    H, W = depth.shape
    fx, fy, cx, cy = _k4(K)
    lo, hi, gap = F32(depth_range[0]), F32(depth_range[1]), F32(max_gap)
    out, valid, image = np.zeros((H, W, 3), F32), np.zeros((H, W), bool), np.zeros((H, W, 3), np.uint8)

    def is_valid(v, u):
        z = depth[v, u]
        return bool(np.isfinite(z) and lo < z and z < hi)

    def point(v, u):
        z = F64(depth[v, u])
        return np.array([(F64(u) - cx) * z / fx, (F64(v) - cy) * z / fy, z], dtype=F64)

    def usable(c, q):
        if not (0 <= q[0] < H and 0 <= q[1] < W) or not is_valid(*q):
            return False
        if labels is not None and same_label and labels[q] != labels[c]:
            return False
        zmax, zmin = max(depth[c], depth[q]), min(depth[c], depth[q])
        return bool(F32(zmax - zmin) <= (F32(gap * zmin) if relative else gap))

    def tangent(c, plus, minus):
        a, b = usable(c, plus), usable(c, minus)
        if a and b:
            return point(*plus) - point(*minus)
        if a:
            return point(*plus) - point(*c)
        if b:
            return point(*c) - point(*minus)
        return None

    with np.errstate(all="ignore"):
        for v in range(H):
            for u in range(W):
                c = (v, u)
                if not is_valid(v, u):
                    continue
                tu = tangent(c, (v, u + step), (v, u - step))
                tv = tangent(c, (v + step, u), (v - step, u))
                if tu is None or tv is None:
                    continue
                nx = tv[1] * tu[2] - tv[2] * tu[1]
                ny = tv[2] * tu[0] - tv[0] * tu[2]
                nz = tv[0] * tu[1] - tv[1] * tu[0]
                L2 = (nx * nx + ny * ny) + nz * nz
                if not (np.isfinite(L2) and L2 > 0):
                    continue
                L = np.sqrt(L2)
                n = np.array([F32(nx / L), F32(ny / L), F32(nz / L)], dtype=F32)
                if sign == "plane":
                    n = -n
                out[v, u], valid[v, u] = n, True
                image[v, u] = (_byte(n[2]), _byte(n[1]), _byte(n[0]))
    return out, valid, image


def normals_vec(depth, K, labels=None, step=1, max_gap=0.05, relative=True, same_label=True, depth_range=(0.0, np.inf), sign="camera"):
    depth = np.asarray(depth, dtype=F32)
    H, W = depth.shape
    fx, fy, cx, cy = _k4(K)
    lo, hi, gap = F32(depth_range[0]), F32(depth_range[1]), F32(max_gap)
    vv, uu = np.divmod(np.arange(H * W), W)
    z = depth.ravel()
    lab = None if labels is None else np.asarray(labels).ravel()
    with np.errstate(all="ignore"):
        ok = np.isfinite(z) & (lo < z) & (z < hi)

        def points(v, u, zq):
            zq = zq.astype(F64)
            return (u.astype(F64) - cx) * zq / fx, (v.astype(F64) - cy) * zq / fy, zq

        def side(dv, du):
            """-> (usable, the neighbour's point) for the neighbour at (v + dv, u + du) of every pixel"""
            qv, qu = vv + dv, uu + du
            inside = (qv >= 0) & (qv < H) & (qu >= 0) & (qu < W)
            q = np.where(inside, qv * W + qu, 0)
            zq = z[q]
            use = ok & inside & ok[q]
            if lab is not None and same_label:
                use = use & (lab[q] == lab)
            zmin = np.minimum(z, zq)
            spread = (np.maximum(z, zq) - zmin).astype(F32)
            bound = (gap * zmin).astype(F32) if relative else gap
            return use & (spread <= bound), points(qv, qu, zq)

        centre = points(vv, uu, z)

        def tangent(plus, minus):
            (a, pa), (b, pb) = plus, minus
            return [np.where(a, pa[i], centre[i]) - np.where(b, pb[i], centre[i]) for i in range(3)], a | b

        tu, has_u = tangent(side(0, step), side(0, -step))
        tv, has_v = tangent(side(step, 0), side(-step, 0))
        nx = tv[1] * tu[2] - tv[2] * tu[1]
        ny = tv[2] * tu[0] - tv[0] * tu[2]
        nz = tv[0] * tu[1] - tv[1] * tu[0]
        L2 = (nx * nx + ny * ny) + nz * nz
        valid = ok & has_u & has_v & np.isfinite(L2) & (L2 > 0)
        L = np.sqrt(L2)
        n = np.stack([(nx / L).astype(F32), (ny / L).astype(F32), (nz / L).astype(F32)], 1)
        if sign == "plane":
            n = -n
        n = np.where(valid[:, None], n, F32(0.0)).astype(F32)
        image = np.where(valid[:, None], np.rint((n[:, ::-1].astype(F64) * 0.5 + 0.5) * 255.0), 0.0).astype(np.uint8)
    return n.reshape(H, W, 3), valid.reshape(H, W), image.reshape(H, W, 3)


def same(x, y):
    """two (normals, valid, ...) results agree bit for bit (floats compared as bits: -0.0 counts)"""
    for p, q in zip(x, y):
        p, q = np.ascontiguousarray(p), np.ascontiguousarray(q)
        if p.shape != q.shape or p.dtype != q.dtype or p.tobytes() != q.tobytes():
            return False
    return True


def thr2_of(thresholds):
    return [(2.0 * np.sin(np.radians(F64(t)) / 2.0)) ** 2 for t in thresholds]


def squared_chords(a, va, b, vb):
    """a, b [...,3] float32, va, vb [...] -> d2 float64 over the pixels valid in both, in row-major order"""
    both = (np.asarray(va).reshape(-1) != 0) & (np.asarray(vb).reshape(-1) != 0)
    d = np.asarray(a, F32).reshape(-1, 3)[both].astype(F64) - np.asarray(b, F32).reshape(-1, 3)[both].astype(F64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def error_tables(a, va, b, vb, thresholds=(11.25, 22.5, 30)):
    """one image pair -> (hist [BINS], within [T], count) int64"""
    d2 = squared_chords(a, va, b, vb)
    bins = np.minimum(BINS - 1, np.floor(np.sqrt(d2) * (BINS // 2))).astype(np.int64)
    return np.bincount(bins, minlength=BINS).astype(np.int64), np.array([(d2 <= t).sum() for t in thr2_of(thresholds)], dtype=np.int64), np.int64(d2.size)


def exact_angles(a, va, b, vb):
    """the angles in degrees of the same chords, without the histogram"""
    return np.degrees(2.0 * np.arcsin(np.minimum(1.0, np.sqrt(squared_chords(a, va, b, vb)) / 2.0)))


def bin_width(i):
    """the width in degrees of histogram bin i"""
    edge = lambda j: np.degrees(2.0 * np.arcsin(min(1.0, j / (BINS / 2.0) / 2.0)))      # noqa: E731
    return edge(i + 1) - edge(i)
