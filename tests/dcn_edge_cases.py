"""TEST INFRASTRUCTURE (not a test): inputs that put DCNv2's sampling points ON the geometric edges of the rule, the bookkeeping that
proves they are there, and a second, switchable restatement of the rule whose deliberate mistakes ("mutants") show that the bounds of
tests/test_dcn_edges_gpu.py would catch them.

The sampling rule exists three times in the library -- `make_tap` (csrc/prn_dcn.hip: offset / modulator gradient, CSR inversion of the
input gradient), `dcnv2_table_body` (csrc/prn_dcnv2.hip: pair-load table of the weight gradient and the gather forward) and
`dcnv2_table2_body` (the per-patch window table of the windowed forward) -- and once in oracle/dcn_ref.py.  Every case here is run
through all of them on identical data.

Every offset, `max_offset` and mask is a multiple of 1/8 (exact in fp32), handed to the references as `.double()`: floor(), the four
bilinear weights and the inside test then come out IDENTICAL in fp32 and fp64, so a comparison measures the kernel's arithmetic and
not on which side of an edge a rounded coordinate fell.  x, w, the upstream gradient and the biases are random fp32 values.

Used by tests/test_dcn_edges_cpu.py (class counts, mutant separation, fp32 oracle inside the bound) and tests/test_dcn_edges_gpu.py."""
import functools

import torch
import torch.nn.functional as F

from oracle.dcn_ref import deform_conv2d_ref

FWD_RTOL = 2e-4          # the bounds of tests/test_ops_gpu.py: max-abs error <= RTOL * max|ref|
GRAD_RTOL = 5e-4
MIN_POINTS = 32          # a class a case claims holds at least this many sampling points
MAX_BIN = 256            # no CSR bin of any case holds more entries (one thread sorts a bin quadratically; these tests are about values)
PATCH = 8                # plan_dcn_fwd2 picks 8 x 8 output patches for the window cases' sizes (see window_case)
WROWS, WPITCH = 32, 40   # the largest window the windowed forward stages in LDS (csrc/prn_dcnv2.hip)

GEOMETRY_RULES = ("trunc", "clamp_corners", "ge_minus1", "no_outside")
RAW_RULES = ("no_clamp", "clamp_pass", "sigmoid_half")


def out_hw(H, W, stride, pad):
    return (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn32(*shape, seed, scale=1.0):
    """random values that ARE fp32 numbers, as float64"""
    return (torch.randn(*shape, generator=_gen(seed), dtype=torch.float64) * scale).float().double()


def grid_offsets(shape, seed, lim):
    """multiples of 1/8 in [-lim, lim], a quarter of them rounded to integers"""
    g = _gen(seed)
    n = int(lim * 8)
    off = torch.randint(-n, n + 1, shape, generator=g).double() / 8
    return torch.where(torch.rand(shape, generator=g) < 0.25, off.round(), off)


def grid_mask(shape, seed):
    """multiples of 1/8 in [0, 2]: exact zeros (and twos) included"""
    return torch.randint(0, 17, shape, generator=_gen(seed)).double() / 8


def base_coords(Ho, Wo, stride, pad):
    """sampling positions at zero offset: y [9, Ho, 1], x [9, 1, Wo] (tap k = 3 * ki + kj)"""
    k = torch.arange(9)
    ki, kj = (k // 3).view(9, 1, 1), (k % 3).view(9, 1, 1)
    by = (torch.arange(Ho).view(1, Ho, 1) * stride - pad + ki).double()
    bx = (torch.arange(Wo).view(1, 1, Wo) * stride - pad + kj).double()
    return by, bx


def sample_coords(offset, stride, pad):
    """the oracle's own geometry: y = ho * s - p + ki + dy, x likewise -> [B, 9, Ho, Wo] each"""
    B, _, Ho, Wo = offset.shape
    by, bx = base_coords(Ho, Wo, stride, pad)
    o = offset.reshape(B, 9, 2, Ho, Wo).double()
    return by + o[:, :, 0], bx + o[:, :, 1]


def plant_edges(off, H, W, stride, pad, seed, lim, per=48, allowed=None):
    """Moves `per` sampling points each exactly onto y = -1, y = H, x = -1 and x = W, and as many into each of the four border bands
    (-1, 0) and (H - 1, H) / (W - 1, W) -- the other coordinate stays strictly inside, so the edge alone decides -- with offsets that
    stay within +-lim.  Disjoint points; `allowed` [B, 9, Ho, Wo] restricts the choice."""
    B, _, Ho, Wo = off.shape
    by, bx = base_coords(Ho, Wo, stride, pad)
    o = off.view(B, 9, 2, Ho, Wo)                        # a view: writes land in `off`
    taken = torch.zeros(B, 9, Ho, Wo, dtype=torch.bool) if allowed is None else ~allowed
    g = _gen(seed)
    for axis, target, band in ((0, -1.0, 0), (0, float(H), 0), (1, -1.0, 0), (1, float(W), 0),
                               (0, -1.0, 1), (0, H - 1.0, 1), (1, -1.0, 1), (1, W - 1.0, 1)):
        y, x = sample_coords(off, stride, pad)
        frac = torch.randint(1, 8, (B, 9, Ho, Wo), generator=g).double() / 8 * band      # band: strictly between the edge and the next pixel
        need = target + frac - (by if axis == 0 else bx)
        other_in = ((x > -1) & (x < W)) if axis == 0 else ((y > -1) & (y < H))
        idx = ((need.abs() <= lim) & other_in & ~taken).flatten().nonzero().flatten()
        idx = idx[torch.randperm(idx.numel(), generator=g)[:per]]
        sel = torch.zeros(B * 9 * Ho * Wo, dtype=torch.bool)
        sel[idx] = True
        sel = sel.view(B, 9, Ho, Wo)
        o[:, :, axis][sel] = need[sel]
        taken |= sel
    return off


# ------------------------------------------------------------------------------------------------ classes of sampling points
def point_classes(y, x, H, W):
    """boolean [B, 9, Ho, Wo] per class, from the sampling coordinates"""
    yin, xin = (y > -1) & (y < H), (x > -1) & (x < W)
    inside = yin & xin
    yi, xi = y == y.floor(), x == x.floor()
    return {
        "y_on_m1": (y == -1) & xin, "y_on_H": (y == H) & xin, "x_on_m1": (x == -1) & yin, "x_on_W": (x == W) & yin,
        "y_low_band": (y > -1) & (y < 0) & xin, "y_high_band": (y > H - 1) & (y < H) & xin,
        "x_low_band": (x > -1) & (x < 0) & yin, "x_high_band": (x > W - 1) & (x < W) & yin,
        "outside": ~inside, "int_one": inside & (yi ^ xi), "int_both": inside & yi & xi,
    }


def raw_classes(om, max_offset):
    """per sampling point [B, 9, Ho, Wo], from the raw 27-channel map: an offset coordinate strictly beyond / exactly on the clamp, a
    saturated modulator logit"""
    B, _, Ho, Wo = om.shape
    o, m = om[:, :18].reshape(B, 9, 2, Ho, Wo), om[:, 18:]
    return {"beyond": (o.abs() > max_offset).any(2), "on_pmax": (o == max_offset).any(2), "on_nmax": (o == -max_offset).any(2),
            "sat_logit": m.abs() >= 20}


def patch_boxes(y, x, H, W, PH=PATCH, PW=PATCH):
    """Bounding box of the live corners per output patch, as dcnv2_table2_body defines it: over the patch's points strictly inside
    (-1, H) x (-1, W), rows min(y0) .. max(y0 + 1) and columns min(x0) .. max(x0 + 1) with (y0, x0) = floor; a patch without a live
    point has a 0 x 0 window.  -> dict of [B, tilesY, tilesX] tensors: wy0, wx0, wh, ww, live (number of live points)."""
    B, _, Ho, Wo = y.shape
    tY, tX = -(-Ho // PH), -(-Wo // PW)
    inside = (y > -1) & (y < H) & (x > -1) & (x < W)
    big = 1 << 30
    res = {k: torch.zeros(B, tY, tX, dtype=torch.long) for k in ("wy0", "wx0", "wh", "ww", "live")}
    y0, x0 = y.floor().long(), x.floor().long()
    for ty in range(tY):
        for tx in range(tX):
            sl = (slice(None), slice(None), slice(ty * PH, (ty + 1) * PH), slice(tx * PW, (tx + 1) * PW))
            live = inside[sl].flatten(1)
            a, c = y0[sl].flatten(1), x0[sl].flatten(1)
            n = live.sum(1)
            ylo, yhi = torch.where(live, a, big).amin(1), torch.where(live, a + 1, -big).amax(1)
            xlo, xhi = torch.where(live, c, big).amin(1), torch.where(live, c + 1, -big).amax(1)
            some = n > 0
            res["live"][:, ty, tx] = n
            res["wy0"][:, ty, tx] = torch.where(some, ylo, 0)
            res["wx0"][:, ty, tx] = torch.where(some, xlo, 0)
            res["wh"][:, ty, tx] = torch.where(some, yhi - ylo + 1, 0)
            res["ww"][:, ty, tx] = torch.where(some, xhi - xlo + 1, 0)
    return res


def window_classes(box, H, W):
    """which window classes of the windowed forward the patches of a case fall into -> dict name -> number of patches"""
    wh, ww = box["wh"], box["ww"]
    area = wh * ww
    staged = (wh <= WROWS) & (ww <= WPITCH) & (box["live"] > 0)
    return {
        "empty": (box["live"] == 0), "nwl1": staged & (area <= 256), "nwl2": staged & (area > 256) & (area <= 512),
        "nwl5": staged & (area > 512), "rows32": staged & (wh == WROWS), "cols40": staged & (ww == WPITCH),
        "rows33": (wh == WROWS + 1), "cols41": (ww == WPITCH + 1), "fallback": (wh > WROWS) | (ww > WPITCH),
        "top": staged & (box["wy0"] == -1), "left": staged & (box["wx0"] == -1),
        "bottom": staged & (box["wy0"] + wh - 1 == H), "right": staged & (box["wx0"] + ww - 1 == W),
    }


def bin_counts(y, x, H, W):
    """entries per CSR bin (image, tap, input pixel) of the input gradient: a sampling point enters the bin of each of its corners
    that lies inside the image with a non-zero bilinear weight -> [B, 9, H * W]"""
    B = y.shape[0]
    inside = (y > -1) & (y < H) & (x > -1) & (x < W)
    y0, x0 = y.floor(), x.floor()
    ly, lx = y - y0, x - x0
    cnt = torch.zeros(B * 9 * H * W, dtype=torch.long)
    plane = (torch.arange(B * 9).view(B, 9, 1, 1) * (H * W)).expand_as(y)
    for cy, wy in ((y0, 1 - ly), (y0 + 1, ly)):
        for cx, wx in ((x0, 1 - lx), (x0 + 1, lx)):
            ok = inside & (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1) & (wy * wx != 0)
            cnt += torch.bincount((plane + (cy * W + cx).long())[ok], minlength=cnt.numel())
    return cnt.view(B, 9, H * W)


# ------------------------------------------------------------------------------------------------ switchable restatement
def dcn_restate(inp, offset, mask, weight, bias, stride, pad, rule="true"):
    """A second statement of torchvision's rule that shares no code with oracle/dcn_ref.py: the image gets a one-pixel ring of zeros, a
    point strictly inside (-1, H) x (-1, W) has all four corners on the ringed image, every other point is dropped.  rule="true" equals
    the oracle to 1e-12 (asserted by tests/test_dcn_edges_cpu.py); the other rules are the plausible mistakes at the edges:
      trunc          (int) cast instead of floor: wrong for coordinates in (-1, 0)
      clamp_corners  corners outside the image read the nearest edge pixel instead of zero
      ge_minus1      -1 counts as inside (value unchanged -- the weight there is 0 -- but the one-sided offset derivative is not)
      no_outside     no inside test at all: only the per-corner validity remains"""
    B, C, H, W = inp.shape
    Ho, Wo = out_hw(H, W, stride, pad)
    y, x = sample_coords(offset, stride, pad)
    y, x = y.to(inp.dtype), x.to(inp.dtype)
    lo = torch.trunc if rule == "trunc" else torch.floor
    y0, x0 = lo(y.detach()), lo(x.detach())
    ly, lx = y - y0, x - x0
    if rule == "ge_minus1":
        inside = (y >= -1) & (y < H) & (x >= -1) & (x < W)
    elif rule == "no_outside":
        inside = torch.ones_like(y, dtype=torch.bool)
    else:
        inside = (y > -1) & (y < H) & (x > -1) & (x < W)
    ring = F.pad(inp, (1, 1, 1, 1), mode="replicate" if rule == "clamp_corners" else "constant")
    flat = ring.reshape(B, C, (H + 2) * (W + 2))
    cols = 0
    for cy, wy in ((y0, 1 - ly), (y0 + 1, ly)):
        for cx, wx in ((x0, 1 - lx), (x0 + 1, lx)):
            on_ring = inside & (cy >= -1) & (cy <= H) & (cx >= -1) & (cx <= W)
            idx = ((cy.clamp(-1, H) + 1) * (W + 2) + cx.clamp(-1, W) + 1).long().view(B, 1, -1).expand(B, C, -1)
            v = torch.gather(flat, 2, idx).view(B, C, 9, Ho, Wo)
            cols = cols + v * (wy * wx * on_ring.to(inp.dtype)).unsqueeze(1)
    if mask is not None:
        cols = cols * mask.unsqueeze(1)
    out = torch.einsum("mck,bckhw->bmhw", weight.reshape(weight.shape[0], C, 9), cols)
    return out if bias is None else out + bias.view(1, -1, 1, 1)


def raw_restate(inp, om, weight, bias, stride, max_offset, rule="true", sampler=dcn_restate):
    """raw mode (models/dcn.py:53-57 folded into the tables): offsets = clamp(om[:, :18], +-max_offset), modulation = 2 * sigmoid(om[:, 18:]).
      no_clamp      the offsets are used as they come
      clamp_pass    the clamp's gradient gate is missing (values clamped, gradient always passed)
      sigmoid_half  the derivative of 2 * sigmoid without its factor 2"""
    o, m = om[:, :18], om[:, 18:]
    if rule == "no_clamp":
        off = o
    elif rule == "clamp_pass":
        off = o + (o.clamp(-max_offset, max_offset) - o).detach()
    else:
        off = o.clamp(-max_offset, max_offset)
    s = torch.sigmoid(m)
    mod = (s + s.detach()) if rule == "sigmoid_half" else 2 * s
    return sampler(inp, off, mod, weight, bias, stride, 1, rule if rule in GEOMETRY_RULES else "true")


def _oracle_sampler(inp, off, mod, weight, bias, stride, pad, rule):
    assert rule == "true"
    return deform_conv2d_ref(inp, off, mod, weight, bias, stride, pad)


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """kind "plain": ops.deform_conv2d semantics, leaves x, off, w, b (+ msk).  kind "raw": the raw [B, 27, Ho, Wo] map, leaves x, om, w, b.
    kind "block": the map is conv3x3(x; w27, b27), leaves x, w27, b27, w, b.  `t` holds the leaves and the upstream gradient `go` as
    float64 tensors with fp32 values; `claims`: classes with >= MIN_POINTS points; `mutants`: the wrong rules that apply to the case."""

    def __init__(self, name, kind, dims, t, claims=(), mutants=(), max_offset=0.0, patch_claims=()):
        self.name, self.kind, self.t, self.claims, self.mutants, self.max_offset, self.patch_claims = name, kind, t, claims, mutants, max_offset, patch_claims
        self.B, self.C, self.H, self.W, self.M, self.stride, self.pad = dims
        self.Ho, self.Wo = out_hw(self.H, self.W, self.stride, self.pad)
        self.leaves = [k for k in ("x", "off", "msk", "om", "w27", "b27", "w", "b") if t.get(k) is not None]

    def forward(self, t, impl="oracle", rule="true"):
        """t: name -> tensor (any float dtype).  impl "oracle": oracle/dcn_ref.py (rule "true" only); "restate": the switchable one."""
        if self.kind == "plain":
            if impl == "oracle":
                return deform_conv2d_ref(t["x"], t["off"], t.get("msk"), t["w"], t["b"], self.stride, self.pad)
            return dcn_restate(t["x"], t["off"], t.get("msk"), t["w"], t["b"], self.stride, self.pad, rule)
        om = t["om"] if self.kind == "raw" else F.conv2d(t["x"], t["w27"], t["b27"], stride=self.stride, padding=1)
        return raw_restate(t["x"], om, t["w"], t["b"], self.stride, self.max_offset, rule, _oracle_sampler if impl == "oracle" else dcn_restate)

    def evaluate(self, dtype=torch.float64, impl="oracle", rule="true"):
        """-> {"y": output, "d_<leaf>": gradient of sum(y * go)} as float64"""
        t = {k: self.t[k].detach().clone().to(dtype).requires_grad_(True) for k in self.leaves}
        y = self.forward(t, impl, rule)
        gs = torch.autograd.grad(y, [t[k] for k in self.leaves], self.t["go"].to(dtype))
        res = {"y": y.detach().double()}
        res.update({"d_" + k: g.double() for k, g in zip(self.leaves, gs)})
        return res

    @functools.lru_cache(maxsize=None)
    def reference(self):
        """the fp64 oracle, computed once and shared (treat as read-only)"""
        return self.evaluate()

    @functools.lru_cache(maxsize=None)
    def raw_map(self):
        """the fp64 [B, 27, Ho, Wo] map of a raw / block case"""
        if self.kind == "raw":
            return self.t["om"]
        return F.conv2d(self.t["x"], self.t["w27"], self.t["b27"], stride=self.stride, padding=1)

    @functools.lru_cache(maxsize=None)
    def coords(self):
        """sampling coordinates after the clamp of raw mode"""
        off = self.t["off"] if self.kind == "plain" else self.raw_map()[:, :18].clamp(-self.max_offset, self.max_offset)
        return sample_coords(off, self.stride, self.pad)

    @functools.lru_cache(maxsize=None)
    def classes(self):
        y, x = self.coords()
        c = point_classes(y, x, self.H, self.W)
        if self.kind != "plain":
            c.update(raw_classes(self.raw_map(), self.max_offset))
        return c

    def counts(self):
        return {k: int(v.sum()) for k, v in self.classes().items()}

    def boxes(self):
        y, x = self.coords()
        return patch_boxes(y, x, self.H, self.W)

    @functools.lru_cache(maxsize=None)
    def bins(self):
        y, x = self.coords()
        return bin_counts(y, x, self.H, self.W)

    def bound(self, name):
        return FWD_RTOL if name == "y" else GRAD_RTOL

    def structural_zeros(self):
        """{gradient name: boolean mask} of entries that no arithmetic can make non-zero: a point outside the image has no offset and no
        modulator gradient, a zero modulator no offset gradient, an offset strictly beyond the clamp none, a logit of +-100 (expf
        overflows / vanishes: the modulation is exactly 0 or 2) none, an input pixel in no bin none."""
        c = self.classes()
        two = lambda m: m.unsqueeze(2).expand(-1, -1, 2, -1, -1).reshape(self.B, 18, self.Ho, self.Wo)
        z = {"d_x": (self.bins().sum(1) == 0).view(self.B, 1, self.H, self.W).expand(-1, self.C, -1, -1)}
        if self.kind == "plain":
            dead = c["outside"] if self.t.get("msk") is None else (c["outside"] | (self.t["msk"] == 0))
            z["d_off"] = two(dead)
            if self.t.get("msk") is not None:
                z["d_msk"] = c["outside"]
        elif self.kind == "raw":
            om = self.t["om"]
            z["d_om"] = torch.cat([two(c["outside"] | (om[:, 18:] <= -100)) | (om[:, :18].abs() > self.max_offset),
                                   c["outside"] | (om[:, 18:].abs() >= 100)], 1)
        return z


def _common(B, C, H, W, M, Ho, Wo, seed):
    return {"x": _randn32(B, C, H, W, seed=seed + 1), "w": _randn32(M, C, 3, 3, seed=seed + 3, scale=(9 * C) ** -0.5),
            "b": _randn32(M, seed=seed + 4), "go": _randn32(B, M, Ho, Wo, seed=seed + 5)}


ALL_POINT_CLASSES = ("y_on_m1", "y_on_H", "x_on_m1", "x_on_W", "y_low_band", "y_high_band", "x_low_band", "x_high_band", "outside", "int_one", "int_both")
EDGE_MIX_SHAPES = {"windowed": (1, 16, 24, 48, 24, 1, 1), "oddC_gather": (2, 5, 9, 11, 5, 1, 0), "stride2_tm2": (2, 16, 31, 33, 72, 2, 1),
                   "tm4": (1, 8, 16, 16, 136, 1, 1)}


def edge_mix_case(name, dims, with_mask, seed, lim=3.0, claims=ALL_POINT_CLASSES, mutants=GEOMETRY_RULES, per=48):
    """offsets on the 1/8 grid within +-lim, a quarter of them integers, 48 points each planted exactly on -1 / H / W and in the border bands, in y and in x"""
    B, C, H, W, M, stride, pad = dims
    Ho, Wo = out_hw(H, W, stride, pad)
    t = _common(B, C, H, W, M, Ho, Wo, seed)
    t["off"] = plant_edges(grid_offsets((B, 18, Ho, Wo), seed + 2, lim), H, W, stride, pad, seed + 7, lim, per)
    t["msk"] = grid_mask((B, 9, Ho, Wo), seed + 6) if with_mask else None
    return Case(name, "plain", dims, t, claims, mutants)


def raw_map_tensor(B, Ho, Wo, max_offset, seed):
    """[B, 27, Ho, Wo]: a third of the offsets strictly beyond +-max_offset (up to 3x), 48 exactly on +max_offset and 48 on -max_offset,
    the rest on the 1/8 grid strictly within (a quarter integers); modulator logits from {0, +-1, +-20, +-100}"""
    g = _gen(seed)
    n = int(max_offset * 8)
    shape = (B, 18, Ho, Wo)
    within = torch.randint(-(n - 1), n, shape, generator=g).double() / 8
    within = torch.where(torch.rand(shape, generator=g) < 0.25, within.round().clamp(-(n - 1) / 8, (n - 1) / 8), within)
    far = (max_offset + torch.randint(1, 2 * n + 1, shape, generator=g).double() / 8) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    off = torch.where(torch.rand(shape, generator=g) < 1 / 3, far, within).flatten()
    pick = torch.randperm(off.numel(), generator=g)[:96]
    off[pick[:48]] = max_offset
    off[pick[48:]] = -max_offset
    levels = torch.tensor([0.0, 1.0, -1.0, 20.0, -20.0, 100.0, -100.0], dtype=torch.float64)
    logit = levels[torch.randint(0, 7, (B, 9, Ho, Wo), generator=g)]
    return torch.cat([off.view(shape), logit], 1)


RAW_CLAIMS = ("beyond", "on_pmax", "on_nmax", "sat_logit", "outside", "int_one")
BAND_CLAIMS = ("y_low_band", "y_high_band", "x_low_band", "x_high_band")      # (claimed at stride 1 only: stride 2 leaves 8 x 8 output pixels per image)


def raw_case(name, stride, seed):
    dims = (2, 16, 16, 16, 24, stride, 1)
    B, C, H, W, M, _, _ = dims
    Ho, Wo = out_hw(H, W, stride, 1)
    t = _common(B, C, H, W, M, Ho, Wo, seed)
    t["om"] = raw_map_tensor(B, Ho, Wo, 2.5, seed + 2)
    return Case(name, "raw", dims, t, RAW_CLAIMS + (BAND_CLAIMS if stride == 1 else ()), ("trunc", "clamp_corners") + RAW_RULES, max_offset=2.5)


def block_case(name, stride, seed):
    """The whole node: the map comes out of the 27-channel conv.  Six of the eighteen offset biases are +-6 (every offset of those
    channels saturates the clamp of 2.5), two modulator biases +-30 (saturated logits)."""
    dims = (2, 16, 16, 16, 24, stride, 1)
    B, C, H, W, M, _, _ = dims
    Ho, Wo = out_hw(H, W, stride, 1)
    t = _common(B, C, H, W, M, Ho, Wo, seed)
    t["w27"] = _randn32(27, C, 3, 3, seed=seed + 8, scale=0.4 * (9 * C) ** -0.5)
    b27 = (_randn32(27, seed=seed + 9, scale=0.3) + 0.125).float().double()
    b27[[0, 5, 7, 10, 12, 17]] = torch.tensor([6.0, -6.0, 6.0, -6.0, 6.0, -6.0], dtype=torch.float64)
    b27[18], b27[19] = 30.0, -30.0
    t["b27"] = b27
    return Case(name, "block", dims, t, ("beyond", "sat_logit", "outside") + (BAND_CLAIMS if stride == 1 else ()),
                ("trunc", "clamp_corners") + RAW_RULES, max_offset=2.5)


def _stretch(off, H, W, stride, b, ty, tx, rows=None, cols=None):
    """Moves ONE sampling point of patch (ty, tx) -- the centre tap of a pixel in its middle -- so that the patch's window gets exactly
    `rows` rows (and another one for `cols` columns): away from the image border that is too close."""
    o = off.view(off.shape[0], 9, 2, off.shape[2], off.shape[3])
    for axis, want, size, pix in ((0, rows, H, 3), (1, cols, W, 4)):
        if want is None:
            continue
        y, x = sample_coords(off, stride, 1)
        box = patch_boxes(y, x, H, W)
        lo = int(box["wy0" if axis == 0 else "wx0"][b, ty, tx])
        hi = lo + int(box["wh" if axis == 0 else "ww"][b, ty, tx]) - 1
        if lo + want - 1 <= size:                               # grow towards larger coordinates: floor = new_hi - 1
            target = lo + want - 1 - 0.5
        else:
            assert hi - want + 1 >= -1, "no room for a window of %d along axis %d" % (want, axis)
            target = hi - want + 1 + 0.5
        ho, wo = ty * PATCH + pix, tx * PATCH + pix
        o[b, 4, axis, ho, wo] = target - (ho if axis == 0 else wo) * stride      # centre tap: base coordinate = pixel * stride
    return off


WINDOW_SPECS = {
    # (ty, tx) -> recipe; "base": fractional offsets in [0, 1) only; patches not listed get edge-mix offsets (+-3) with planted edge points
    1: {(0, 0): {"rows": 33}, (0, 1): {"cols": 41}, (1, 0): {"rows": 32}, (1, 1): {"cols": 40}, (1, 2): {"rows": 24, "cols": 24},
        (2, 2): {"empty": True}, (3, 5): {"rows": 32, "cols": 40}, (4, 1): {"rows": 33, "cols": 41},
        (0, 3): {}, (2, 0): {}, (2, 5): {}, (4, 3): {}},
    2: {(0, 0): {"rows": 33}, (0, 1): {}, (0, 2): {"cols": 41}, (1, 0): {"rows": 32, "cols": 40}, (1, 1): {"empty": True},
        (1, 2): {"contract": True}, (2, 0): {"rows": 32}, (2, 2): {}},
}
WINDOW_PATCH_CLAIMS = ("empty", "nwl1", "nwl2", "nwl5", "rows32", "cols40", "rows33", "cols41", "top", "left", "bottom", "right")


def window_case(name, stride, seed):
    """One patch per window class of the windowed forward.  These cases are aimed at the 8 x 8 output patches plan_dcn_fwd2 picks for the
    sizes used here (40 x 48 outputs at stride 1, 24 x 24 at stride 2: of the four candidate shapes 8 x 8 gives the fewest patches, or ties
    and comes first); patch_boxes() restates the window of such a patch."""
    dims = (1, 16, 40, 48, 24, 1, 1) if stride == 1 else (1, 16, 48, 48, 24, 2, 1)
    B, C, H, W, M, _, _ = dims
    Ho, Wo = out_hw(H, W, stride, 1)
    assert Ho % PATCH == 0 and Wo % PATCH == 0
    t = _common(B, C, H, W, M, Ho, Wo, seed)
    specs = WINDOW_SPECS[stride]
    off = grid_offsets((B, 18, Ho, Wo), seed + 2, 3.0)
    frac = torch.randint(0, 8, (B, 18, Ho, Wo), generator=_gen(seed + 8)).double() / 8
    filler = torch.ones(B, 9, Ho, Wo, dtype=torch.bool)
    for (ty, tx), spec in specs.items():
        sl = (slice(None), slice(None), slice(ty * PATCH, (ty + 1) * PATCH), slice(tx * PATCH, (tx + 1) * PATCH))
        filler[sl] = False
        off[sl] = frac[sl]
        if spec.get("empty"):
            off[sl] = 64.0                                      # all 576 points far outside
        if spec.get("contract"):                                # stride 2: pull the patch's rows / columns together to stride 1
            py = torch.arange(PATCH, dtype=torch.float64)
            off[sl][:, 0::2] -= py.view(1, 1, PATCH, 1) * (stride - 1)
            off[sl][:, 1::2] -= py.view(1, 1, 1, PATCH) * (stride - 1)
    plant_edges(off, H, W, stride, 1, seed + 7, 3.0, allowed=filler)
    for (ty, tx), spec in specs.items():
        _stretch(off, H, W, stride, 0, ty, tx, spec.get("rows"), spec.get("cols"))
    t["off"] = off
    t["msk"] = grid_mask((B, 9, Ho, Wo), seed + 6)
    claims = ("outside", "y_low_band", "y_high_band", "x_low_band", "x_high_band", "int_one")
    return Case(name, "plain", dims, t, claims, GEOMETRY_RULES if stride == 1 else ("trunc", "clamp_corners"), patch_claims=WINDOW_PATCH_CLAIMS)


def csr_convergence_case(name="csr_convergence", seed=500):
    """Image 0: all 256 points of every tap go to ONE fractional location (four bins of 256 entries per tap plane, every other bin empty).
    Image 1: per tap, a seeded permutation of the 256 points is cut into groups of 8, 9, 8, 9, ... points; group g goes to its own
    fractional location on a lattice of pitch 2 (footprints do not overlap): bins of exactly 8 and exactly 9 entries, the two sides of
    the sorting network's limit.  The one point left over is sent outside."""
    dims = (2, 8, 16, 16, 8, 1, 1)
    B, C, H, W, M, stride, pad = dims
    Ho, Wo = out_hw(H, W, stride, pad)
    t = _common(B, C, H, W, M, Ho, Wo, seed)
    by, bx = base_coords(Ho, Wo, stride, pad)
    ty = torch.zeros(B, 9, Ho, Wo, dtype=torch.float64)
    tx = torch.zeros(B, 9, Ho, Wo, dtype=torch.float64)
    g = _gen(seed + 2)
    for k in range(9):
        ty[0, k], tx[0, k] = 2 + k + 0.375, 12 - k + 0.625
        perm = torch.randperm(Ho * Wo, generator=g)
        gy, gx = torch.full((Ho * Wo,), 80.0, dtype=torch.float64), torch.full((Ho * Wo,), 80.0, dtype=torch.float64)
        pos = 0
        for grp in range(30):
            n = 8 if grp % 2 == 0 else 9
            gy[perm[pos:pos + n]] = 2 * (grp // 8) + 0.375 + 0.125 * (k % 3)
            gx[perm[pos:pos + n]] = 2 * (grp % 8) + 0.625
            pos += n
        ty[1, k], tx[1, k] = gy.view(Ho, Wo), gx.view(Ho, Wo)
    t["off"] = torch.stack([ty - by, tx - bx], 2).reshape(B, 18, Ho, Wo)
    t["msk"] = grid_mask((B, 9, Ho, Wo), seed + 6).clamp(min=0.125)
    return Case(name, "plain", dims, t, (), ())


def csr_switch_case(name, H):
    """H * W = 15360 is the last map whose CSR structure is built in one launch (a tap plane's bins in LDS), 97 x 160 the first built in five"""
    return edge_mix_case(name, (1, 2, H, 160, 4, 1, 1), True, 600 + H)


NARROW_SHAPES = {"1x1": (1, 1), "5x1": (5, 1), "3x2": (3, 2), "2x2": (2, 2)}


def narrow_case(name):
    """maps narrower than the pixel pair the pair-load table fetches; too few points for class claims"""
    H, W = NARROW_SHAPES[name.split("_")[1]]
    return edge_mix_case(name, (16, 4, H, W, 6, 1, 1), True, 700 + 10 * H + W, lim=1.5, claims=(), mutants=("trunc", "clamp_corners"), per=6)


BUILDERS = {}
for _i, (_n, _d) in enumerate(EDGE_MIX_SHAPES.items()):
    BUILDERS["mix_%s_nomask" % _n] = functools.partial(edge_mix_case, "mix_%s_nomask" % _n, _d, False, 100 + 20 * _i)
    BUILDERS["mix_%s_mask0" % _n] = functools.partial(edge_mix_case, "mix_%s_mask0" % _n, _d, True, 110 + 20 * _i)
for _s in (1, 2):
    BUILDERS["raw_s%d" % _s] = functools.partial(raw_case, "raw_s%d" % _s, _s, 200 + _s)
    BUILDERS["block_s%d" % _s] = functools.partial(block_case, "block_s%d" % _s, _s, 300 + _s)
    BUILDERS["window_s%d" % _s] = functools.partial(window_case, "window_s%d" % _s, _s, 400 + _s)
BUILDERS["csr_convergence"] = csr_convergence_case
BUILDERS["csr_hw15360"] = functools.partial(csr_switch_case, "csr_hw15360", 96)
BUILDERS["csr_hw15520"] = functools.partial(csr_switch_case, "csr_hw15520", 97)
for _n in NARROW_SHAPES:
    BUILDERS["narrow_" + _n] = functools.partial(narrow_case, "narrow_" + _n)

EDGE_MIX = [n for n in BUILDERS if n.startswith("mix_")]
RAW = ["raw_s1", "raw_s2"]
BLOCK = ["block_s1", "block_s2"]
WINDOW = ["window_s1", "window_s2"]
CSR_SWITCH = ["csr_hw15360", "csr_hw15520"]
NARROW = ["narrow_" + n for n in NARROW_SHAPES]


@functools.lru_cache(maxsize=None)
def get_case(name):
    """cases (and their fp64 references) are built once per process and shared by the tests"""
    return BUILDERS[name]()


def rel_err(got, ref):
    """(max-abs error / max|ref|, max|ref|)"""
    den = ref.abs().max().item() + 1e-300
    return (got.double() - ref).abs().max().item() / den, den


def per_class_report(case, got, ref):
    """maximum error per class of sampling point, relative to the tensor maximum: the output at pixels that own a point of the class, the
    offset / modulator gradients at the points themselves -- so that a failure names the edge"""
    lines = []
    for cname, m in sorted(case.classes().items()):
        if not m.any():
            continue
        parts = []
        e = (got["y"].double() - ref["y"]).abs().amax(1) / (ref["y"].abs().max().item() + 1e-300)              # [B, Ho, Wo]
        parts.append("y %.2e" % e[m.any(1)].max().item())
        for g in ("d_off", "d_msk", "d_om"):
            if g not in got or g not in ref:
                continue
            d = (got[g].double() - ref[g]).abs() / (ref[g].abs().max().item() + 1e-300)
            if g == "d_msk":
                d = d[m]
            elif g == "d_off":
                d = d.view(case.B, 9, 2, case.Ho, case.Wo).amax(2)[m]
            else:
                d = torch.maximum(d[:, :18].reshape(case.B, 9, 2, case.Ho, case.Wo).amax(2), d[:, 18:])[m]
            parts.append("%s %.2e" % (g, d.max().item()))
        lines.append("    %-12s %6d points: %s" % (cname, int(m.sum()), ", ".join(parts)))
    return "\n".join(lines)
