"""numpy-only restatement of planerecnet_amd.components (connected-component labels, mask cleaning) in two independent forms, and the
hand-made masks the tests and tests/golden/make_golden_components.py share.

  label_flood     a flood fill with an explicit stack from every unlabelled set pixel in row-major order (pure Python over a padded list)
  (label_flood_batch: the same over a batch; the cheaper of the two, so the reference of the GPU tests)
  label_minprop   every set pixel starts with its own row-major index and takes the minimum over its neighbours until nothing changes; the
                  surviving values, ranked, are the labels
Both number the components 1..K in ascending order of their first pixel in row-major order (scipy.ndimage.label's order).  `clean` restates the
selection and the hole filling from labels of either form.
"""
import numpy as np

NEIGHBOURS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)), 8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def label_flood(mask, connectivity=8):
    """mask [H,W] -> (labels int32 [H,W], K)"""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    Wp = W + 2
    pad = np.zeros((H + 2, Wp), np.uint8)
    pad[1:-1, 1:-1] = mask
    flat = pad.ravel().tolist()
    lab = [0] * len(flat)
    offs = [dy * Wp + dx for dy, dx in NEIGHBOURS[connectivity]]
    k = 0
    for start in np.flatnonzero(pad.ravel()).tolist():
        if lab[start]:
            continue
        k += 1
        lab[start] = k
        stack = [start]
        while stack:
            p = stack.pop()
            for o in offs:
                q = p + o
                if flat[q] and not lab[q]:
                    lab[q] = k
                    stack.append(q)
    return np.asarray(lab, np.int32).reshape(H + 2, Wp)[1:-1, 1:-1].copy(), k


def label_flood_batch(masks, connectivity=8):
    """masks [N,H,W] -> (labels int32 [N,H,W], K int32 [N]) by label_flood"""
    masks = np.asarray(masks)
    res = [label_flood(m, connectivity) for m in masks]
    labels = np.stack([lab for lab, _ in res]) if res else np.zeros(masks.shape, np.int32)
    return labels, np.asarray([k for _, k in res], np.int32)


def label_minprop(masks, connectivity=8):
    """masks [H,W] or [N,H,W] -> (labels int32 of the same shape, K int or int32 [N])"""
    masks = np.asarray(masks) != 0
    single = masks.ndim == 2
    m = masks[None] if single else masks
    N, H, W = m.shape
    big = H * W
    lab = np.where(m, np.arange(H * W, dtype=np.int64).reshape(1, H, W), big)
    active = np.arange(N)                                            # masks that changed in the last round
    while active.size:
        cur = lab[active]
        pad = np.full((active.size, H + 2, W + 2), big, np.int64)
        pad[:, 1:-1, 1:-1] = cur
        new = cur
        for dy, dx in NEIGHBOURS[connectivity]:
            new = np.minimum(new, pad[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        new = np.where(m[active], new, big)
        changed = (new != cur).reshape(active.size, -1).any(1)
        lab[active] = new
        active = active[changed]
    out = np.zeros((N, H, W), np.int32)
    count = np.zeros(N, np.int32)
    for n in range(N):
        firsts = np.unique(lab[n][m[n]])
        count[n] = firsts.size
        out[n][m[n]] = np.searchsorted(firsts, lab[n][m[n]]) + 1
    return (out[0], int(count[0])) if single else (out, count)


def _label_batch(label, masks, connectivity):
    if label is label_minprop:
        return label(masks, connectivity)                            # (one fixed-point iteration for the whole batch)
    res = [label(m, connectivity) for m in masks]
    return [lab for lab, _ in res], [k for _, k in res]


def clean_batch(masks, connectivity=8, keep="largest", min_area=0, fill_holes=False, label=label_minprop):
    """[N,H,W] -> (cleaned bool [N,H,W], dict of int32 [N] count / kept / largest / area), from the labels of `label`"""
    masks = np.asarray(masks) != 0
    N = masks.shape[0]
    sel = np.zeros(masks.shape, bool)
    info = {k: np.zeros(N, np.int32) for k in ("count", "kept", "largest", "area")}
    if N == 0:
        return sel, info
    labs, counts = _label_batch(label, masks, connectivity)
    for n in range(N):
        K = int(counts[n])
        areas = np.bincount(labs[n].ravel(), minlength=K + 1)[1:].tolist()
        chosen = []
        if keep == "largest":
            if K and max(areas) >= min_area:
                chosen = [areas.index(max(areas)) + 1]               # (index: the first maximum = the lowest label)
        else:
            chosen = [k for k in range(1, K + 1) if areas[k - 1] >= min_area]
        sel[n] = np.isin(labs[n], chosen)
        info["count"][n], info["kept"][n], info["largest"][n] = K, len(chosen), max(areas) if K else 0
    if fill_holes:
        backs, _ = _label_batch(label, ~sel, 4 if connectivity == 8 else 8)
        for n in range(N):
            back = backs[n]
            outside = set(back[0].tolist()) | set(back[-1].tolist()) | set(back[:, 0].tolist()) | set(back[:, -1].tolist())
            outside.discard(0)
            sel[n] |= (back > 0) & ~np.isin(back, sorted(outside))
    info["area"][:] = sel.reshape(N, -1).sum(1)
    return sel, info


def clean(mask, connectivity=8, keep="largest", min_area=0, fill_holes=False, label=label_minprop):
    """mask [H,W] -> (cleaned bool [H,W], dict of ints)"""
    sel, info = clean_batch(np.asarray(mask)[None], connectivity, keep, min_area, fill_holes, label)
    return sel[0], {k: int(v[0]) for k, v in info.items()}


# what the fixture and the tests run every mask through: (keep, min_area, fill_holes)
CLEAN_VARIANTS = (("largest", 0, False), ("largest", 0, True), ("all", 0, True), ("all", 5, False), ("all", 5, True), ("largest", 10 ** 6, True))


def _outline(m, y0, y1, x0, x1):
    """the one-pixel outline of the rectangle rows y0..y1, columns x0..x1 (inclusive), clipped to the image; nothing if it is empty"""
    H, W = m.shape
    y0, x0, y1, x1 = max(y0, 0), max(x0, 0), min(y1, H - 1), min(x1, W - 1)
    if y1 < y0 or x1 < x0:
        return
    m[y0, x0:x1 + 1] = True
    m[y1, x0:x1 + 1] = True
    m[y0:y1 + 1, x0] = True
    m[y0:y1 + 1, x1] = True


def _block(m, y0, x0, h, w):
    H, W = m.shape
    m[max(y0, 0):max(min(y0 + h, H), 0), max(x0, 0):max(min(x0 + w, W), 0)] = True


def patterns(H, W, tile=(32, 64), densities=(0.1, 0.5, 0.59, 0.9), seed=0):
    """name -> bool [H,W]: the smallest shapes at which each phase of the device path can go wrong (any H, W >= 1; at tiny sizes the
    shapes are clipped, which still makes valid inputs)"""
    TH, TW = tile
    z = lambda: np.zeros((H, W), bool)      # noqa: E731
    yy, xx = np.mgrid[:H, :W]
    P = {"empty": z(), "full": ~z()}
    m = z()
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = True
    P["corners"] = m
    m = z()
    d = np.arange(min(H, W))
    m[d, d] = True                                                   # K = 1 for 8, K = length for 4
    P["diagonal"] = m
    P["checker"] = (yy + xx) % 2 == 0                                # one component for 8, every pixel its own for 4
    P["hstripes"] = yy % 2 == 0
    P["vstripes"] = xx % 2 == 0
    # serpentines: full even rows (columns) joined at alternating ends -- one chain that crosses every vertical (horizontal) seam on every other row
    P["serpentine"] = (yy % 2 == 0) | ((yy % 2 == 1) & np.where((yy // 2) % 2 == 0, xx == W - 1, xx == 0))
    P["serpentine_v"] = (xx % 2 == 0) | ((xx % 2 == 1) & np.where((xx // 2) % 2 == 0, yy == H - 1, yy == 0))
    # square spiral: a walk that turns right whenever the cell ahead is outside, set, or next to an earlier arm -- one chain, arms one pixel apart
    m = z()
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    inside = lambda a, b: 0 <= a < H and 0 <= b < W      # noqa: E731
    turned = False
    while True:
        ny, nx = y + dy, x + dx
        if inside(ny, nx) and not m[ny, nx] and not (inside(ny + dy, nx + dx) and m[ny + dy, nx + dx]):
            y, x, turned = ny, nx, False
            m[y, x] = True
        elif turned:
            break
        else:
            dy, dx, turned = dx, -dy, True
    P["spiral"] = m
    # two U-shapes that meet only at a tile corner: diagonal contact (one component for 8, two for 4), on both diagonals
    cy, cx = (TH if H > TH else H // 2), (TW if W > TW else W // 2)
    for name, flip in (("ucorner", False), ("ucorner_anti", True)):
        a, b = z(), z()
        _outline(a, cy - 4, cy - 1, cx - 4, cx - 1)
        if cy - 4 >= 0:
            a[cy - 4, max(cx - 3, 0):max(cx - 1, 0)] = False          # open at the top
        _outline(b, cy, cy + 3, cx, cx + 3)
        if cy + 3 < H:
            b[cy + 3, cx + 1:cx + 3] = False                         # open at the bottom
        if flip:                                                     # mirror both about the seam column: contact (cy-1, cx) ~ (cy, cx-1)
            a2, b2 = z(), z()
            for src, dst in ((a, a2), (b, b2)):
                ys, xs = np.nonzero(src)
                xs = 2 * cx - 1 - xs
                ok = (xs >= 0) & (xs < W)
                dst[ys[ok], xs[ok]] = True
            a, b = a2, b2
        P[name] = a | b
    m = z()
    _outline(m, 1, H - 2, 1, W - 2)
    P["ring"] = m
    m = z()                                                          # nested rings, an island with its own hole inside
    _outline(m, 1, H - 2, 1, W - 2)
    _outline(m, 3, H - 4, 3, W - 4)
    if H >= 13 and W >= 13:
        _block(m, 5, 5, H - 10, W - 10)
        m[H // 2, W // 2] = False
    P["nested"] = m
    m = z()                                                          # the "hole" reaches the border through the gap in the top edge
    _outline(m, 0, H - 2, 1, W - 2)
    m[0, W // 2] = False
    P["open_hole"] = m
    m = z()                                                          # a hole that holds a speck
    _outline(m, 1, H - 2, 1, W - 2)
    m[H // 2, W // 2] = True
    P["speck_in_hole"] = m
    m = z()                                                          # two / three components of equal maximal area (and a smaller one before them)
    m[0, W - 1] = True
    _block(m, 2, 1, 2, 3)
    _block(m, H - 3, W - 4, 2, 3)
    P["tie2"] = m
    m = m.copy()
    _block(m, H // 2, W // 2 - 1, 2, 3)
    P["tie3"] = m
    m = z()                                                          # areas 6, 4 and 1: min_area 5, 6, 7 sit below, at and above the largest
    _block(m, 0, 0, 2, 3)
    _block(m, H - 2, W - 2, 2, 2)
    m[H // 2, W // 2] = True
    P["areas_6_4_1"] = m
    rng = np.random.RandomState(seed + 131 * H + W)
    for dens in densities:                                           # 0.59: near the 4-connected percolation threshold (long ragged components)
        P["random_%g" % dens] = rng.rand(H, W) < dens
    return P


def blobs(seed, n, H, W, specks=12, pinholes=12):
    """n masks: a filled ellipse each, with specks outside it and pin-holes inside it (what a thresholded, resized SOLO mask looks like)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((n, H, W), bool)
    for i in range(n):
        cy, cx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W
        ry, rx = rng.uniform(0.08, 0.3) * H + 1, rng.uniform(0.08, 0.3) * W + 1
        m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        inside = np.flatnonzero(m)
        for _ in range(specks):
            y, x = rng.randint(H), rng.randint(W)
            m[y:y + rng.randint(1, 4), x:x + rng.randint(1, 4)] = True
        if inside.size:
            for p in rng.choice(inside, min(pinholes, inside.size), replace=False):
                y, x = divmod(int(p), W)
                m[y:y + rng.randint(1, 3), x:x + rng.randint(1, 3)] = False
        out[i] = m
    return out


def load_fixture(path):
    """tests/golden/components_cases.npz -> {tag: dict(names, masks bool [N,H,W], labels {conn: int32 [N,H,W]}, count {conn: int32 [N]},
    clean {(conn, variant): bool [N,H,W]}, info {(conn, variant): int32 [4,N] = count, kept, largest, area})}"""
    z = np.load(path)
    out = {}
    for tag in sorted(k[6:] for k in z.files if k.startswith("names_")):
        N, H, W = (int(v) for v in z["shape_" + tag])
        unpack = lambda a: np.unpackbits(a)[:N * H * W].reshape(N, H, W).astype(bool)      # noqa: E731
        c = {"names": [str(s) for s in z["names_" + tag]], "masks": unpack(z["masks_" + tag]), "labels": {}, "count": {}, "clean": {}, "info": {}}
        for conn in (4, 8):
            c["labels"][conn] = z["labels%d_%s" % (conn, tag)].astype(np.int32)
            c["count"][conn] = z["count%d_%s" % (conn, tag)]
            for v in range(len(CLEAN_VARIANTS)):
                c["clean"][conn, v] = unpack(z["clean%d_v%d_%s" % (conn, v, tag)])
                c["info"][conn, v] = z["info%d_v%d_%s" % (conn, v, tag)]
        out[tag] = c
    return out
