"""fp64 restatement of the robust plane fit (include/prn.h: prn_planes_ransac_fit) in numpy: Philox4x32-10 and the
seven rules of the contract -- draws, hypothesis, score, choice, refit, refine, result -- with planes_restate.restate for every
least-squares fit.  Used by tests/test_planes_ransac_cpu.py and tests/test_planes_ransac_gpu.py, which share the fuzz references below.

restate_ransac also counts the UNDECIDED tests of a call, on the instances it finds valid: (pixel, plane) pairs with
| |n . X - d| - t | <= 1e-9 t, and hypotheses whose c . c is within a factor 1 +- 1e-6 of the degeneracy bound.  Where that count is 0, fp64
rounding (FMA contraction, the eigen-solver) cannot change an inlier set or a chosen hypothesis, and the device must agree exactly."""
import functools

import numpy as np

from planes_restate import k_of, plane_depth_map, restate

_M0, _M1, _W0, _W1, _LO = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four, key: two arrays (or scalars) of 32-bit values -> four uint64 arrays holding the 32-bit output words"""
    c0, c1, c2, c3 = [np.atleast_1d(np.asarray(c, np.uint64)) & _LO for c in np.broadcast_arrays(*counter)]
    k0, k1 = [np.asarray(k, np.uint64) & _LO for k in key]
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0, c1, c2, c3


def _points(depth, k_matrix):
    H, W = depth.shape
    k = np.asarray(k_matrix, np.float64)
    fx, cx, fy, cy = k[0, 0], k[0, 2], k[1, 1], k[1, 2]
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    Z = depth.astype(np.float64)
    with np.errstate(all="ignore"):
        return np.stack([(u - cx) * Z / fx, (v - cy) * Z / fy, Z], -1).reshape(-1, 3)


def _within(pts, plane, threshold, relative):
    """(inliers [n, k] bool, undecided [k] int) of points [n,3] against planes [k,4]"""
    with np.errstate(all="ignore"):
        r = np.abs(pts[:, :1] * plane[None, :, 0] + pts[:, 1:2] * plane[None, :, 1] + pts[:, 2:3] * plane[None, :, 2] - plane[None, :, 3])
        t = threshold * pts[:, 2:3] if relative else np.full((pts.shape[0], 1), threshold)
        fin = np.isfinite(pts[:, 2:3])
        inl = (r <= t) & fin
        und = (np.abs(r - t) <= 1e-9 * t) & fin
    return inl, und.sum(0)


def _lsq(depth, sets, k_matrix):
    _, planes, valid = restate(depth, sets, k_matrix)
    return planes.numpy().copy(), valid.numpy().copy()


def restate_ransac(depth, masks, k_matrix, threshold=0.05, relative=False, hypotheses=256, refine=1, seed=0):
    """depth [H,W] fp32, masks [N,H,W] bool, k_matrix [3,3]; the instance index within the image is the mask's index ->
    dict(planes [N,4], valid [N], count [N], inliers [N], hypothesis [N], inlier_masks [N,H,W] bool, undecided int)"""
    depth = np.asarray(depth, np.float32)
    masks = np.asarray(masks).astype(bool)
    N, H, W = masks.shape
    pts = _points(depth, k_matrix)
    flat = masks.reshape(N, -1)
    count = flat.sum(1).astype(np.int64)
    hyp = np.full(N, -1, np.int32)
    sets = np.zeros((N, H * W), bool)
    undecided = np.zeros(N, np.int64)
    hs = np.arange(hypotheses, dtype=np.uint64)
    for i in range(N):
        idx = np.flatnonzero(flat[i])
        if idx.size == 0:
            continue
        w = philox4x32_10((hs, 0, i, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        p = [pts[idx[((w[j] * np.uint64(idx.size)) >> _S32).astype(np.int64)]] for j in range(3)]           # rule 1
        with np.errstate(all="ignore"):                                                                  # rule 2
            e1, e2 = p[1] - p[0], p[2] - p[0]
            c = np.cross(e1, e2)
            cc, bound = (c * c).sum(1), 1e-12 * ((e1 * e1).sum(1) * (e2 * e2).sum(1))
            ok = cc > bound
            n = c / np.sqrt(cc)[:, None]
            planes = np.concatenate([n, (n * p[0]).sum(1, keepdims=True)], 1)
            # (bound == 0: a draw repeats p0, so e1 or e2 and with it c is exactly zero in any arithmetic -- decided, not close)
            undecided[i] += int(((bound > 0) & (np.abs(cc - bound) <= 1e-6 * bound)).sum())
        planes[~ok] = np.nan
        inl, und = _within(pts[idx], planes, threshold, relative)                                        # rule 3
        score = inl.sum(0)
        undecided[i] += int(und[ok].sum())
        h = int(np.argmax(score))                                                                        # rule 4: the lowest index of the largest
        if score[h] < 3:
            continue
        hyp[i] = h
        sets[i, idx[inl[:, h]]] = True
    planes, valid = _lsq(depth, sets.reshape(N, H, W), k_matrix)                                         # rule 5
    for _ in range(refine):                                                                              # rule 6
        for i in range(N):
            sets[i] = False
            if valid[i]:
                idx = np.flatnonzero(flat[i])
                inl, und = _within(pts[idx], planes[i:i + 1], threshold, relative)
                undecided[i] += int(und[0])
                sets[i, idx[inl[:, 0]]] = True
        planes, valid = _lsq(depth, sets.reshape(N, H, W), k_matrix)
    sets[~valid] = False                                                                                 # rule 7
    hyp[~valid] = -1
    planes[~valid] = np.nan
    return {"planes": planes, "valid": valid, "count": count, "inliers": sets.sum(1).astype(np.int64), "hypothesis": hyp,
            "inlier_masks": sets.reshape(N, H, W), "undecided": int(undecided[valid].sum())}


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------------

DOMINANT = (np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0]), 2.5)
SECOND = (np.array([-0.6, 0.1, 1.0]) / np.linalg.norm([-0.6, 0.1, 1.0]), 1.6)


def two_plane_scene(H, W, frac=0.25, seed=0):
    """(depth [H,W] fp32, mask [1,H,W] bool, K, dominant region [H,W] bool): the dominant plane, the left frac * W columns on the second plane,
    0.5 % multiplicative noise; a full-frame mask with 5 % of its pixels dropped"""
    rng = np.random.RandomState(seed)
    K = k_of(0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 - 0.5)
    depth = plane_depth_map(DOMINANT[0], DOMINANT[1], K, H, W)
    cut = int(round(frac * W))
    depth[:, :cut] = plane_depth_map(SECOND[0], SECOND[1], K, H, W)[:, :cut]
    depth = depth * (1 + 0.005 * rng.randn(H, W))
    mask = (rng.rand(H, W) > 0.05)[None]
    region = np.zeros((H, W), bool)
    region[:, cut:] = True
    return depth.astype(np.float32), mask, K, region


def angle_deg(n, ref):
    return float(np.degrees(np.arccos(min(1.0, abs(float(np.dot(n, ref)))))))


# (N, H, W, hypotheses, relative, refine) of the device fuzz; threshold and seed are the same for all
FUZZ = [(1, 60, 80, 1, False, 0), (7, 37, 53, 64, False, 1), (100, 60, 80, 100, True, 1), (100, 45, 67, 256, False, 2), (7, 33, 31, 4096, False, 1)]
FUZZ_THRESHOLD, FUZZ_SEED = 0.02, 5


def fuzz_input(N, H, W):
    """the masks and depth of test_planes_gpu's fuzz, from its generator"""
    from test_planes_gpu import _fuzz_image
    rng = np.random.RandomState(1000 * N + H)
    K = k_of(70.0 + rng.rand() * 20, 70.0 + rng.rand() * 20, W / 2 - 0.5, H / 2 - 0.5)
    depth, masks = _fuzz_image(rng, N, H, W, K)
    return depth, masks, K


@functools.lru_cache(maxsize=None)
def fuzz_reference(cfg, seed=FUZZ_SEED):
    """(depth, masks, K, restatement) of one FUZZ configuration: computed once per process, shared by the tests; treat as read-only"""
    N, H, W, hypotheses, relative, refine = cfg
    depth, masks, K = fuzz_input(N, H, W)
    return depth, masks, K, restate_ransac(depth, masks, K, threshold=FUZZ_THRESHOLD, relative=relative, hypotheses=hypotheses, refine=refine, seed=seed)
