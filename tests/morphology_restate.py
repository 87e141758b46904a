"""Independent numpy restatements of planerecnet_amd/morphology.py and of the boundary IoU / boundary AP of planerecnet_amd/metrics.py, the
pattern generator of the morphology tests and the reader of tests/golden/boundary_cases.npz.

Two restatements of the erosion, neither separable, neither by doubling (the two things the product does):
  erode_views   the definition: pad with `border`, AND of the (2r+1)^2 shifted views.  (2r+1)^2 passes: used for small radii.
  erode         the same set by counting: a pixel survives iff the (2r+1)^2 window of the padded mask holds (2r+1)^2 set pixels, the count
                taken from a summed-area table.  One pass whatever r is, so the GPU tests can afford r = max(H, W) + 7.
tests/test_morphology_cpu.py holds both against each other and against scipy.ndimage.  A radius beyond max(H, W) is clamped to it: such a
window already holds the whole image and a border on every side."""
import numpy as np


def _pad(m, r, border):
    return np.pad(np.asarray(m, bool), ((0, 0), (r, r), (r, r)), constant_values=bool(border))


def erode_views(m, r, border=0):
    """m [N,H,W] bool"""
    m = np.asarray(m, bool)
    N, H, W = m.shape
    r = min(int(r), max(H, W))
    p = _pad(m, r, border)
    out = np.ones((N, H, W), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out &= p[:, dy:dy + H, dx:dx + W]
    return out


def dilate_views(m, r, border=0):
    m = np.asarray(m, bool)
    N, H, W = m.shape
    r = min(int(r), max(H, W))
    p = _pad(m, r, border)
    out = np.zeros((N, H, W), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= p[:, dy:dy + H, dx:dx + W]
    return out


def _window_counts(m, r, border):
    """number of set pixels in the (2r+1)^2 window round every pixel of the bordered mask, and the window's size"""
    m = np.asarray(m, bool)
    N, H, W = m.shape
    r = min(int(r), max(H, W))
    n = 2 * r + 1
    p = _pad(m, r, border)
    S = np.zeros((N, H + 2 * r + 1, W + 2 * r + 1), np.int32)          # (a count is at most the padded mask's size: far below 2^31 at any test size)
    S[:, 1:, 1:] = p.cumsum(1, dtype=np.int32).cumsum(2, dtype=np.int32)
    return S[:, n:n + H, n:n + W] - S[:, :H, n:n + W] - S[:, n:n + H, :W] + S[:, :H, :W], n * n


def erode(m, r, border=0):
    c, full = _window_counts(m, r, border)
    return c == full


def dilate(m, r, border=0):
    c, _ = _window_counts(m, r, border)
    return c > 0


def erode_dilate(m, r, border=0):
    """both from one table"""
    c, full = _window_counts(m, r, border)
    return c == full, c > 0


def boundary(m, r):
    m = np.asarray(m, bool)
    return m & ~erode(m, r, 0)


def iou_f32(a, b):
    """[A,H,W] x [B,H,W] bool -> [A,B] fp32: inter / ((|a| + |b|) - inter), every operand and operation fp32 (0/0 = NaN)"""
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    fa, fb = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    inter = (fa[:, None, :] & fb[None, :, :]).sum(2).astype(np.float32)
    aa, ab = fa.sum(1).astype(np.float32), fb.sum(1).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (inter / ((aa[:, None] + ab[None, :]) - inter)).astype(np.float32)


def boundary_ious(a, b, r):
    """-> (mask IoU, boundary IoU) of two mask sets, fp32"""
    return iou_f32(a, b), iou_f32(boundary(a, r), boundary(b, r))


def ap_pushes(iou, scores, thr):
    """What match_frame pushes for one threshold: the detections in descending score order, each as a miss, a matched one (some IoU of its
    row above thr; NaN never) as a hit before that -- [(score, hit), ...]"""
    scores = np.asarray(scores, np.float64)
    out = []
    for i in np.argsort(-scores, kind="stable"):
        if iou.shape[1] and bool((iou[i] > thr).any()):
            out.append((float(scores[i]), True))
        out.append((float(scores[i]), False))
    return out


def boundary_ap_iou(mask_iou, boundary_iou):
    return np.minimum(mask_iou, boundary_iou)


# ---- patterns --------------------------------------------------------------------------------------------------------------------

def blobs(seed, n, H, W, specks=6, pinholes=6):
    """n masks: a filled ellipse each, with specks outside it and pin-holes inside it (what a thresholded, resized SOLO mask looks like)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((n, H, W), bool)
    for i in range(n):
        cy, cx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W
        ry, rx = rng.uniform(0.1, 0.45) * H + 1, rng.uniform(0.1, 0.45) * W + 1
        m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        inside = np.flatnonzero(m)
        for _ in range(specks):
            y, x = rng.randint(H), rng.randint(W)
            m[y:y + rng.randint(1, 4), x:x + rng.randint(1, 4)] = True
        for p in rng.choice(inside, min(pinholes, inside.size), replace=False) if inside.size else ():
            y, x = divmod(int(p), W)
            m[y, x] = False
        out[i] = m
    return out


RECT_RADII = (1, 2, 3, 31, 32, 33, 64)


def patterns(H, W, seed=0):
    """{name: [H,W] bool}: empty, full, single pixels, checkerboard, a one-pixel frame, for every r of RECT_RADII that fits a rectangle exactly
    2r+1 wide and high (one pixel survives erode(r)), 2r+1 x 2r (nothing survives) and 2r+1 x (2r+3) (a line survives), touching no edge
    where there is room, and seeded blobs with pin-holes."""
    P = {}
    z = np.zeros((H, W), bool)
    P["empty"] = z.copy()
    P["full"] = ~z
    for name, (y, x) in (("px_tl", (0, 0)), ("px_tr", (0, W - 1)), ("px_bl", (H - 1, 0)), ("px_br", (H - 1, W - 1)), ("px_c", (H // 2, W // 2))):
        P[name] = z.copy()
        P[name][y, x] = True
        P["hole_" + name[3:]] = ~P[name]
    yy, xx = np.mgrid[:H, :W]
    P["checker"] = (yy + xx) % 2 == 0
    P["frame"] = z.copy()
    P["frame"][[0, -1], :] = True
    P["frame"][:, [0, -1]] = True
    for r in RECT_RADII:
        n = 2 * r + 1
        for tag, (h, w) in (("sq", (n, n)), ("short", (n - 1, n)), ("narrow", (n, n - 1)), ("line", (n, n + 2))):
            if h <= H and w <= W:
                y0, x0 = min(1, H - h), min(1, W - w)
                P["rect%d_%s" % (r, tag)] = z.copy()
                P["rect%d_%s" % (r, tag)][y0:y0 + h, x0:x0 + w] = True
    for i, b in enumerate(blobs(100 + seed, 3, H, W)):
        P["blob%d" % i] = b
    return P


def pattern_batch(H, W, seed=0):
    P = patterns(H, W, seed)
    return np.stack([P[k] for k in sorted(P)]), sorted(P)


# ---- the shifted-rectangle frame of the boundary AP tests --------------------------------------------------------------------------

def shifted_rectangles():
    """-> (gt [1,96,128], det [3,96,128], scores): one ground-truth plane, rows 10..69 x columns 20..99, and three detections shifted by 0, 1
    and 2 pixels in both axes.  With r = 3: mask IoU 1, 0.9437, 0.8913; boundary IoU 1, 0.5028, 0.2072.  The worse a detection, the higher
    its score: a missed detection then stands before the hits and lowers the AP (with the exact one first every AP would be 100)."""
    gt = np.zeros((1, 96, 128), bool)
    gt[0, 10:70, 20:100] = True
    det = np.zeros((3, 96, 128), bool)
    for s in range(3):
        det[s, 10 + s:70 + s, 20 + s:100 + s] = True
    return gt, det, np.array([0.7, 0.8, 0.9])


def load_fixture(path):
    """tests/golden/boundary_cases.npz -> {tag: {"masks" [N,H,W] bool, "radii", "erode" {(r, border): [N,H,W]}, "dilate" {...}, "band" {r: ...},
    "split", "mask_iou" {r: [A,B]}, "boundary_iou" {r: [A,B]}}}; the IoU matrices are of masks[:split] against masks[split:]"""
    z = np.load(path)
    out = {}
    for tag in [k[6:] for k in z.files if k.startswith("shape_")]:
        N, H, W = (int(v) for v in z["shape_" + tag])
        unpack = lambda a: np.unpackbits(a)[:N * H * W].reshape(N, H, W).astype(bool)      # noqa: E731
        radii = [int(r) for r in z["radii_" + tag]]
        c = {"masks": unpack(z["masks_" + tag]), "radii": radii, "split": int(z["split_" + tag]), "erode": {}, "dilate": {}, "band": {},
             "mask_iou": {}, "boundary_iou": {}}
        for r in radii:
            for b in (0, 1):
                c["erode"][r, b] = unpack(z["erode_%s_r%d_b%d" % (tag, r, b)])
                c["dilate"][r, b] = unpack(z["dilate_%s_r%d_b%d" % (tag, r, b)])
            c["band"][r] = unpack(z["band_%s_r%d" % (tag, r)])
            c["mask_iou"][r] = z["miou_%s_r%d" % (tag, r)]
            c["boundary_iou"][r] = z["biou_%s_r%d" % (tag, r)]
        out[tag] = c
    return out
