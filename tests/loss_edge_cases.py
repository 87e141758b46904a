"""TEST INFRASTRUCTURE (not a test): inputs that put the three fused loss kernels of csrc/prn_loss.hip -- prn_focal_sum_*, prn_rmse_log_*
and prn_mask_loss_* -- on their saturated, boundary and launch-shape edges, the bookkeeping that proves the inputs are there, an fp64
reference, and a switchable restatement of each formula whose deliberate mistakes ("rules") show that the bounds of
tests/test_loss_edges_gpu.py would catch them.

Pure torch on the CPU: this module does not import planerecnet_amd (it has to import without the HIP library).  The three formulas of
planerecnet_amd/losses.py are restated here twice: `plain_*` is the operator chain as written there (sigmoid_focal_sum, rmse_log, dice_loss
and the lava term as in test_fused_mask_loss_matches_operator_chain), `*_restated` is written cell by cell the way the kernels index their
data and takes `rule=`.  Under rule "true" the two agree to 1e-12 (tests/test_loss_edges_cpu.py).

Every input is a number fp32 holds exactly, stored as float64 (`v.float().double() == v`); that includes `min_depth` = float32(0.1) and the
clamp = float32(1e-9), the values the kernels receive: a comparison measures the kernel's arithmetic, not on which side of an edge a rounded
input fell.  `Case.reference()` is the value(s) and the input gradient by fp64 autograd under a non-unit upstream gradient; it is computed
once per case and shared.

Bounds (the project's bound for these kernels, tests/test_model_gpu.py and tests/test_ops_gpu.py: 1e-5):
  scalars    |got - ref| <= 1e-5 |ref|
  gradients  max-abs error <= 1e-5 x scale, with scale = the tensor's max |ref| (focal), each IMAGE's max |ref| (RMSE-log: a whole-tensor
             scale would hide the images with small gradients), per ROW max(row max |ref|, 1e-4 x tensor max |ref|) (mask loss; the floor
             only decides which rows are judged on their own scale)
  structural zeros (pixels without ground truth, predictions below the clamp, the lava gradient when no image qualifies): 0.0 exactly
The fp32 operator chain on the CPU stays within a quarter of these bounds on every case (measured by tests/test_loss_edges_cpu.py, largest
over the cases: focal gradient 1.44e-6 and value 1.3e-7, RMSE-log gradient 2.7e-7 and value 2.1e-7, mask-loss gradient 1.25e-6 -- on the
row of mask_P9_HW4 whose Dice terms nearly cancel -- and scalars 1.5e-7), so no case needs a wider bound than the project's 1e-5.

Deliberately NOT covered:
  * gamma < 1: both the operator chain and the kernel evaluate q^(gamma-1) * 0 = inf * 0 at q = 0.
  * non-finite inputs.  Known difference, not tested here: the kernels' fmaxf(NaN, clamp) returns the clamp where torch.clamp propagates NaN.
  * mask-loss rows that are not laid out image by image (the wrapper's contract requires that order).
  * the virtual-normal kernels (prn_vnl_*): a follow-up.
In the focal size cases the positives include the first row, the last row and the last class; the case past the reduction grid's cap instead
ends in three wrong-side saturated negative cells (x = +30), so that a dropped tail moves the sum -- with C = 2 the last row cannot be both."""
import functools

import torch
import torch.nn.functional as F

BOUND = 1e-5             # every check of tests/test_loss_edges_gpu.py (see above)
ROW_FLOOR = 1e-4         # mask loss: rows whose max |ref| is below this fraction of the tensor maximum are judged on the floor
MIN_CELLS = 8            # an element class a case claims holds at least this many elements

MIN_DEPTH = float(torch.tensor(0.1, dtype=torch.float32))      # what the kernel compares with: float32(0.1)
CLAMP = float(torch.tensor(1e-9, dtype=torch.float32))         # float32(1e-9)
NEXT_ABOVE_MIN_DEPTH = float(torch.nextafter(torch.tensor(0.1, dtype=torch.float32), torch.tensor(1.0)))
GO_FOCAL, GO_RMSE, GO_MASK = 0.375, 5.0, (0.7, 1.9)            # upstream gradients
W_INS, W_LAV = 3.0, 1.0

FOCAL_CAP_CELLS = 131072     # 128 blocks x 1024 cells: beyond, the partial kernel's grid-stride loop runs more than once
RMSE_CAP_PIXELS = 262144     # 128 blocks x 2048 pixels per image

LADDER = (0.0, 1.0, 8.0, 12.0, 15.0, 16.0, 16.5, 16.75, 17.0, 17.5, 20.0, 30.0, 40.0, 60.0, 80.0, 87.0, 88.0, 89.0, 100.0, 104.0, 120.0)
SAT_LOGITS = (20.0, 40.0, 90.0, 120.0)

FOCAL_RULES = ("grad_vanishes_at_pt0", "tail_dropped", "alpha_wrong_side", "gamma_fixed_2", "background_is_last_class", "x_transposed")
RMSE_RULES = ("valid_ge", "strict_clamp_grad", "grad_below_clamp", "mean_all_hw", "images_ge64_dropped", "coef_image0", "tail_dropped")
MASK_RULES = ("last_split_dropped", "rows_ge256_dropped", "eps_once", "lava_mean_over_B", "adj_image0", "dB_sign_flipped")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f32(v):
    """rounded to numbers fp32 holds, as float64"""
    return v.float().double()


# ------------------------------------------------------------------------------------------------ the formulas as losses.py writes them
def plain_focal(x, labels, alpha, gamma):
    C = x.shape[1]
    t = F.one_hot(labels, C + 1)[:, :C].to(x.dtype)
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    loss = ce * (1 - p_t) ** gamma
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss.sum()


def plain_rmse_log(pred, gt, min_depth, clamp):
    n = pred.shape[0]
    valid = gt > min_depth
    l1 = (torch.log(pred.reshape(n, -1).clamp(min=clamp)) - torch.log(gt.reshape(n, -1).clamp(min=clamp))).abs().mul(valid.reshape(n, -1))
    return torch.sqrt((l1 ** 2).sum(1) / valid.reshape(n, -1).sum(1)).mean()


def plain_dice(p, t):
    p = p.reshape(p.shape[0], -1)
    t = t.reshape(t.shape[0], -1).to(p.dtype)
    return 1 - 2 * (p * t).sum(1) / ((p * p).sum(1) + 0.001 + (t * t).sum(1) + 0.001)


def plain_mask(z, t, img, adj, gsum, npos, w_ins, w_lav):
    p = torch.sigmoid(z)
    ins = plain_dice(p, t).mean() * w_ins
    if adj is None:
        return ins, torch.zeros((), dtype=z.dtype)
    num = torch.zeros(adj.shape[0], dtype=z.dtype).index_add_(0, img, (p * adj[img]).flatten(1).sum(1))
    ok = (gsum > 0) & (npos > 0)
    lav = torch.where(ok, num / (gsum * npos).clamp(min=1e-30), torch.zeros_like(num)).sum() / ok.sum().clamp(min=1) * w_lav
    return ins, lav


# ------------------------------------------------------------------------------------------------ the switchable restatements
def focal_restated(x, labels, alpha, gamma, rule="true"):
    """cell (r, c) of x[rows, C]: positive iff labels[r] == c (background: labels[r] == C)"""
    rows, C = x.shape
    xx = x.reshape(C, rows).t() if rule == "x_transposed" else x
    lab = labels.clamp(max=C - 1) if rule == "background_is_last_class" else labels
    pos = lab.view(-1, 1) == torch.arange(C).view(1, C)
    g = 2.0 if rule == "gamma_fixed_2" else gamma
    p = torch.sigmoid(xx)
    ce = -F.logsigmoid(torch.where(pos, xx, -xx))                     # -log p_t
    q = 1 - torch.where(pos, p, 1 - p)
    loss = ce * q ** g
    if alpha >= 0:
        a = 1 - alpha if rule == "alpha_wrong_side" else alpha
        loss = torch.where(pos, torch.full_like(p, a), torch.full_like(p, 1 - a)) * loss
    if rule == "tail_dropped":
        return loss.reshape(-1)[:FOCAL_CAP_CELLS].sum()
    return loss.sum()


def focal_dead_cells(x, labels):
    """cells whose p_t is 0 in fp32 (the gradient the kernel formed as (...) / p_t * p (1 - p) vanished there)"""
    C = x.shape[1]
    pos = labels.view(-1, 1) == torch.arange(C).view(1, C)
    p32 = torch.sigmoid(x.float())
    return torch.where(pos, p32 == 0, (1 - p32) == 0)


def rmse_restated(pred, gt, min_depth, clamp, rule="true"):
    """pred, gt [B, HW]"""
    B, HW = pred.shape
    valid = (gt >= min_depth) if rule == "valid_ge" else (gt > min_depth)
    if rule == "tail_dropped":
        valid = valid & (torch.arange(HW) < RMSE_CAP_PIXELS).view(1, HW)
    pc = pred.clamp(min=clamp)
    if rule == "grad_below_clamp":
        pc = pred + (pc - pred).detach()
    if rule == "strict_clamp_grad":
        pc = torch.where(pred == clamp, pc.detach(), pc)
    d = torch.log(pc) - torch.log(gt.clamp(min=clamp))
    v = valid.to(pred.dtype)
    S = (d * d * v).sum(1)
    n = torch.full_like(S, float(HW)) if rule == "mean_all_hw" else v.sum(1)
    r = torch.sqrt(S / n)
    value = r[:64].sum() / B if rule == "images_ge64_dropped" else r.sum() / B
    if rule == "coef_image0":                                          # d value / d S_b = 1 / (2 B r_b n_b): image 0's for every image
        sur = (S * (1.0 / (2.0 * B * r[0] * n[0])).detach()).sum()
        value = value.detach() + sur - sur.detach()
    return value


def mask_restated(z, t, img, adj, gsum, npos, w_ins, w_lav, rule="true"):
    """z [P, HW] logits, t [P, HW] 0 / 1, img [P] image of the row, adj [B, HW], gsum / npos [B]"""
    P, HW = z.shape
    p, tf = torch.sigmoid(z), t.to(z.dtype)
    keep = torch.ones(HW, dtype=z.dtype)
    if rule == "last_split_dropped":                                   # the partial kernel's fourth quarter of the row's float4 groups
        keep[4 * ((HW // 4) * 3 // 4):] = 0
    a, b, c = (p * tf * keep).sum(1), (p * p * keep).sum(1), (tf * tf * keep).sum(1)
    D = b + c + (0.001 if rule == "eps_once" else 0.002)
    if rule == "dB_sign_flipped":
        D = D.detach() - (b - b.detach())
    dice = 1 - 2 * a / D
    ins = (dice[:256] if rule == "rows_ge256_dropped" else dice).sum() / P * w_ins
    if adj is None:
        return ins, torch.zeros((), dtype=z.dtype)
    B = adj.shape[0]
    A = adj[torch.zeros_like(img)] if rule == "adj_image0" else adj[img]
    num = torch.zeros(B, dtype=z.dtype).index_add_(0, img, (p * A * keep).sum(1))
    ok = (gsum > 0) & (npos > 0)
    per = torch.where(ok, num / (gsum * npos).clamp(min=1e-30), torch.zeros_like(num))
    den = B if rule == "lava_mean_over_B" else ok.sum().clamp(min=1)
    return ins, per.sum() / den * w_lav


# ------------------------------------------------------------------------------------------------ error metrics (relative error, scale)
def scalar_err(got, ref):
    got, ref = float(got), float(ref)
    if ref == 0.0:
        return (0.0 if got == 0.0 else float("inf")), 0.0
    return abs(got - ref) / abs(ref), abs(ref)


def tensor_err(got, ref):
    den = ref.abs().max().item()
    return (got - ref).abs().max().item() / den, den


def group_err(got, ref, floor=0.0):
    """got, ref [G, n]: the largest over the groups of (group's max-abs error / max(group's max |ref|, floor x tensor max |ref|)) and the scale of
    that group; a group whose scale is 0 has to be exact"""
    e, s = (got - ref).abs().amax(1), ref.abs().amax(1)
    s = torch.maximum(s, torch.full_like(s, floor * ref.abs().max().item()))
    rel = torch.where(s > 0, e / s.clamp(min=1e-300), torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float("inf"))))
    if bool(torch.isnan(rel).any()):
        return float("nan"), float("nan")
    k = int(rel.argmax())
    return rel[k].item(), s[k].item()


class Case:
    """family in {"focal", "rmse", "mask"}; t: the inputs (float64 holding fp32 numbers, integer tensors as they are); claims: {class: minimum count}"""
    leaf = {"focal": "x", "rmse": "pred", "mask": "z"}
    grad_name = {"focal": "d_x", "rmse": "d_pred", "mask": "d_logits"}

    def __init__(self, family, name, t, par, claims, cnt, nan_value=False):
        self.family, self.name, self.t, self.par, self.claims, self._counts, self.nan_value = family, name, t, par, claims, cnt, nan_value
        self._ref = None

    # -- evaluation
    def _values(self, leaf, t, impl, rule):
        cast = lambda k: None if t.get(k) is None else t[k].to(leaf.dtype)
        if self.family == "focal":
            f = plain_focal if impl == "plain" else functools.partial(focal_restated, rule=rule)
            return {"value": f(leaf, t["labels"], self.par["alpha"], self.par["gamma"])}
        if self.family == "rmse":
            if impl == "plain":
                B, H, W = self.par["B"], self.par["H"], self.par["W"]
                return {"value": plain_rmse_log(leaf.view(B, 1, H, W), cast("gt").view(B, 1, H, W), MIN_DEPTH, CLAMP)}
            return {"value": rmse_restated(leaf, cast("gt"), MIN_DEPTH, CLAMP, rule)}
        args = (leaf, t["labels"], t["img"], cast("adj"), cast("gsum"), cast("npos"), W_INS, W_LAV)
        ins, lav = plain_mask(*args) if impl == "plain" else mask_restated(*args, rule=rule)
        return {"ins": ins, "lav": lav}

    def evaluate(self, dtype=torch.float64, rule="true", impl="restate"):
        """{scalar(s), input gradient} as float64 CPU tensors, computed in `dtype` by autograd"""
        assert rule == "true" or impl == "restate"
        base = "true" if rule == "grad_vanishes_at_pt0" else rule
        leaf = self.t[self.leaf[self.family]].to(dtype).clone().requires_grad_(True)
        out = self._values(leaf, self.t, impl, base)
        if self.family == "mask":
            total = GO_MASK[0] * out["ins"] + GO_MASK[1] * out["lav"]
        else:
            total = out["value"] * (GO_FOCAL if self.family == "focal" else GO_RMSE)
        g, = torch.autograd.grad(total, leaf)
        g = g.detach().double()
        if rule == "grad_vanishes_at_pt0":
            g = torch.where(focal_dead_cells(self.t["x"], self.t["labels"]), torch.zeros_like(g), g)
        res = {k: v.detach().double() for k, v in out.items()}
        res[self.grad_name[self.family]] = g
        return res

    def reference(self, rule="true"):
        if rule != "true":
            return self.evaluate(rule=rule)
        if self._ref is None:
            self._ref = self.evaluate()
        return self._ref

    # -- bookkeeping
    def counts(self):
        return dict(self._counts)

    def rules(self):
        """the wrong rules that change something on this case"""
        p, t = self.par, self.t
        if self.nan_value:
            return ()
        if self.family == "focal":
            on = {"grad_vanishes_at_pt0": bool(focal_dead_cells(t["x"], t["labels"]).any()), "tail_dropped": p["rows"] * p["C"] > FOCAL_CAP_CELLS,
                  "alpha_wrong_side": p["alpha"] >= 0, "gamma_fixed_2": p["gamma"] != 2.0, "background_is_last_class": bool((t["labels"] == p["C"]).any()),
                  "x_transposed": p["C"] > 1 and p["rows"] > 1}
            return tuple(r for r in FOCAL_RULES if on[r])
        if self.family == "rmse":
            valid = t["gt"] > MIN_DEPTH
            on = {"valid_ge": bool((t["gt"] == MIN_DEPTH).any()), "strict_clamp_grad": bool(((t["pred"] == CLAMP) & valid).any()),
                  "grad_below_clamp": bool(((t["pred"] < CLAMP) & valid).any()), "mean_all_hw": bool((~valid).any()), "images_ge64_dropped": p["B"] > 64,
                  "coef_image0": p["B"] > 1, "tail_dropped": p["H"] * p["W"] > RMSE_CAP_PIXELS}
            return tuple(r for r in RMSE_RULES if on[r])
        lava = t["adj"] is not None
        ok = int(((t["gsum"] > 0) & (t["npos"] > 0)).sum()) if lava else 0
        on = {"last_split_dropped": True, "rows_ge256_dropped": p["P"] > 256, "eps_once": True, "lava_mean_over_B": lava and 0 < ok < p["B"],
              "adj_image0": lava and ok > 0 and bool((t["img"] > 0).any()), "dB_sign_flipped": True}
        return tuple(r for r in MASK_RULES if on[r])

    def structural_zeros(self):
        """{quantity: mask of entries that have to be 0.0 exactly}"""
        if self.family == "rmse":
            return {"d_pred": ~(self.t["gt"] > MIN_DEPTH) | (self.t["pred"] < CLAMP)}
        return {}

    def metric(self, k, got, ref):
        """(relative error, scale) of quantity k under the GPU test's metric"""
        if k in ("value", "ins", "lav"):
            return scalar_err(got, ref)
        if self.family == "focal":
            return tensor_err(got, ref)
        if self.family == "rmse":
            return group_err(got, ref)
        return group_err(got, ref, ROW_FLOOR)

    def bound(self, k):
        return BOUND

    def quantities(self):
        return (["ins", "lav"] if self.family == "mask" else ["value"]) + [self.grad_name[self.family]]


# ------------------------------------------------------------------------------------------------ focal cases
def _focal_ladder(name, alpha, gamma, seed):
    """512 x 2 cells = one reduction block.  Every rung x sign sits on MIN_CELLS positive cells (rows 0 .. 335, alternating class) and on MIN_CELLS
    negative cells (the background rows 336 .. 503, alternating class); the rest is randn * 3."""
    rows, C = 512, 2
    x = _f32(torch.randn(rows, C, generator=_gen(seed), dtype=torch.float64) * 3)
    labels = torch.full((rows,), C, dtype=torch.int64)
    vals = [s * m for m in LADDER for s in (1.0, -1.0) for _ in range(MIN_CELLS)]
    n = len(vals)
    planted = torch.zeros(rows, C, dtype=torch.bool)
    for k, v in enumerate(vals):
        labels[k] = k % 2
        x[k, k % 2] = v
        planted[k, k % 2] = True
        x.view(-1)[n * C + k] = v
        planted.view(-1)[n * C + k] = True
    labels[rows - 1] = C - 1
    pos = labels.view(-1, 1) == torch.arange(C).view(1, C)
    cnt, claims = {}, {}
    for m in LADDER:
        for s, sg in ((1.0, "+"), (-1.0, "-")):
            for kind, sel in (("pos", pos), ("neg", ~pos)):
                here = planted & sel & (x == s * m)
                key = "%s:%s%g" % (kind, sg, m)
                cnt[key] = int(here.sum())
                claims[key] = MIN_CELLS
                for c in range(C):
                    cnt[key + ":class%d" % c] = int(here[:, c].sum())
                    claims[key + ":class%d" % c] = MIN_CELLS // 2
    return Case("focal", name, {"x": x, "labels": labels}, {"rows": rows, "C": C, "alpha": alpha, "gamma": gamma}, claims, cnt)


def _focal_size(name, rows, C, alpha, gamma, seed, tail=False):
    g = _gen(seed)
    x = _f32(torch.randn(rows, C, generator=g, dtype=torch.float64) * 3)
    labels = torch.full((rows,), C, dtype=torch.int64)
    some = torch.randperm(rows, generator=g)[:rows // 10]
    labels[some] = torch.randint(0, C, (some.numel(),), generator=g)
    labels[0] = 0
    if tail:                                                           # the last three cells: negative, x = +30 (C = 2: rows - 2 is positive in class 0)
        labels[rows - 1], labels[rows - 2], labels[rows - 3] = C, 0, C - 1
        x.view(-1)[-3:] = 30.0
    else:
        labels[rows - 1] = C - 1
    pos = labels.view(-1, 1) == torch.arange(C).view(1, C)
    cnt = {"cells": rows * C, "positives": int(pos.sum()), "background_rows": int((labels == C).sum()), "first_row_positive": int(pos[0].any()),
           "last_row_positive": int(pos[-1].any()), "last_class_positives": int(pos[:, C - 1].sum()),
           "tail_wrong_side": int(((x.view(-1)[-3:] == 30.0) & ~pos.view(-1)[-3:]).sum())}
    return Case("focal", name, {"x": x, "labels": labels}, {"rows": rows, "C": C, "alpha": alpha, "gamma": gamma}, {}, cnt)


# ------------------------------------------------------------------------------------------------ RMSE-log cases
def _rmse_case(name, B, H, W, seed, edges=True, on_clamp=False, no_valid=False, tail=False):
    """Image 0 carries the value edges (MIN_CELLS pixels each), image 1 (B >= 3) has exactly one valid pixel, the last image (B >= 3) has
    pred / gt = 1e4; the fraction of pixels without ground truth differs per image."""
    HW = H * W
    g = _gen(seed)
    gt = _f32(torch.rand(B, HW, generator=g, dtype=torch.float64) * 5 + 0.2)
    pred = _f32((gt * (1 + 0.3 * torch.randn(B, HW, generator=g, dtype=torch.float64))).abs() + 0.05)
    frac = 0.2 + 0.5 * torch.arange(B, dtype=torch.float64).view(B, 1) / B
    gt[torch.rand(B, HW, generator=g, dtype=torch.float64) < frac] = 0.0
    gt[:, 0], pred[:, 0] = 1.0, 1.5                                    # every image keeps a valid pixel with a clear error
    if tail:
        gt[:, RMSE_CAP_PIXELS:], pred[:, RMSE_CAP_PIXELS:] = 2.0, 6.0
    cls = {}
    if edges or on_clamp:
        idx = 1 + torch.randperm(HW - 1, generator=g)[:7 * MIN_CELLS].view(7, MIN_CELLS)
        if edges:
            gt[0, idx[0]] = MIN_DEPTH
            gt[0, idx[1]] = NEXT_ABOVE_MIN_DEPTH
            gt[0, idx[2]] = 0.0
            gt[0, idx[3:6].reshape(-1)] = 2.0
            pred[0, idx[3]], pred[0, idx[4]], pred[0, idx[5]] = 0.0, -1.5, float(torch.tensor(1e-30, dtype=torch.float32))
            cls.update({"gt_on_min_depth": idx[0], "gt_next_above_min_depth": idx[1], "gt_zero": idx[2], "pred_zero": idx[3], "pred_negative": idx[4],
                        "pred_tiny": idx[5]})
        if on_clamp:
            gt[0, idx[6]], pred[0, idx[6]] = 2.0, CLAMP
            cls["pred_on_clamp"] = idx[6]
    if B >= 3:
        gt[1] = 0.0
        if not no_valid:
            gt[1, HW // 2], pred[1, HW // 2] = 1.5, 3.0
        pred[B - 1] = _f32(gt[B - 1] * 1e4)
    valid = gt > MIN_DEPTH
    cnt = {"valid_per_image": valid.sum(1).tolist(), "pixels_without_gt": int((~valid).sum())}
    below = (pred[0] < CLAMP) & valid[0]
    checks = {"gt_on_min_depth": ~valid[0] & (gt[0] == MIN_DEPTH), "gt_next_above_min_depth": valid[0] & (gt[0] == NEXT_ABOVE_MIN_DEPTH), "gt_zero": gt[0] == 0,
              "pred_zero": below & (pred[0] == 0), "pred_negative": below & (pred[0] < 0), "pred_tiny": below & (pred[0] > 0),
              "pred_on_clamp": valid[0] & (pred[0] == CLAMP)}
    claims = {}
    for k, where in cls.items():
        cnt[k] = int(checks[k][where].sum())
        claims[k] = MIN_CELLS
    return Case("rmse", name, {"pred": pred, "gt": gt}, {"B": B, "H": H, "W": W}, claims, cnt, nan_value=no_valid)


# ------------------------------------------------------------------------------------------------ mask-loss cases
ROW_KINDS = ("right", "wrong", "empty_target", "all_ones_target")


def _mask_case(name, rows, fh, fw, seed, dice_only=False, gsum0=(), no_qualifying=False, saturated=False):
    """rows[b] = number of rows of image b, laid out image by image"""
    B, P, HW = len(rows), sum(rows), fh * fw
    g = _gen(seed)
    img = torch.repeat_interleave(torch.arange(B), torch.tensor(rows))
    z = _f32(torch.randn(P, HW, generator=g, dtype=torch.float64) * 2)
    t = (torch.rand(P, HW, generator=g) < 0.3).to(torch.uint8)
    adj = _f32(torch.rand(B, HW, generator=g, dtype=torch.float64))
    gsum = _f32(adj.sum(1) * 16.0)
    for b in gsum0:
        adj[b], gsum[b] = 0.0, 0.0
    if no_qualifying:
        gsum[:] = 0.0                                                  # (adj stays: the zero has to come from the qualification test)
    npos = torch.tensor(rows, dtype=torch.float64)
    if HW == 4:
        # a row on which the second 0.001 of the Dice denominator shows: one target pixel with p = 0.905, the others at p = 0.0025, so D = b + c + 0.002
        # = 1.82 and the target pixel's two Dice terms dA + dB p = N / D^2, N = 4 a p - 2 D = -0.37, nearly cancel: 0.001 less in D moves that gradient,
        # the row's largest, by 0.002 (1 / N + 1 / D) = -4e-3 of itself (the fp32 rounding of dA and dB, 2 / D each, moves it by ~1e-6)
        z[0], t[0] = torch.tensor([2.25, -6.0, -6.0, -6.0], dtype=torch.float64), torch.tensor([1, 0, 0, 0], dtype=torch.uint8)
    cnt, claims = {}, {}
    if saturated:
        unsat = torch.zeros(P, HW, dtype=torch.bool)
        mag = torch.tensor(SAT_LOGITS, dtype=torch.float64)[torch.arange(HW) % 4].view(1, HW).expand(P, HW)
        for i in range(P):
            unsat[i, torch.randperm(HW, generator=g)[:MIN_CELLS + i % 5]] = True
            kind = ROW_KINDS[i % 4]
            if kind == "wrong":
                t[i, unsat[i]] = 0                                     # p -> 0 on ALL target pixels
            elif kind == "empty_target":
                t[i] = 0
            elif kind == "all_ones_target":
                t[i] = 1
        sign = (2.0 * t.double() - 1.0)
        kinds = torch.arange(P) % 4
        sign[kinds == 1] *= -1.0
        z = torch.where(unsat, z, sign * mag)
        for k, kind in enumerate(ROW_KINDS):
            cnt["rows_" + kind] = int((kinds == k).sum())
            claims["rows_" + kind] = MIN_CELLS
        for m in SAT_LOGITS:
            for s, sg in ((1.0, "+"), (-1.0, "-")):
                cnt["logit%s%g" % (sg, m)] = int((~unsat & (z == s * m)).sum())
                claims["logit%s%g" % (sg, m)] = MIN_CELLS
        cnt["min_unsaturated_per_row"] = int((z.abs() < 20).sum(1).min())
        claims["min_unsaturated_per_row"] = MIN_CELLS
        cnt["target_pixels_of_wrong_rows_above_-20"] = int(((t == 1) & (z > -20))[kinds == 1].sum())
    ok = (gsum > 0) & (npos > 0)
    cnt.update({"rows_per_image": list(rows), "qualifying_images": 0 if dice_only else int(ok.sum()), "images_gsum0": int((gsum == 0).sum()),
                "images_npos0": int((npos == 0).sum())})
    tt = {"z": z, "labels": t, "img": img, "adj": None if dice_only else adj, "gsum": None if dice_only else gsum, "npos": None if dice_only else npos}
    return Case("mask", name, tt, {"P": P, "B": B, "fh": fh, "fw": fw, "HW": HW}, claims, cnt)


def _spread(P, B):
    """P rows over B images, image by image, uneven"""
    w = [3, 1, 4, 2][:B]
    rows = [P * k // sum(w) for k in w]
    rows[0] += P - sum(rows)
    return rows


CONFIGS = ((0.25, 2.0), (-1.0, 1.5), (0.25, 1.0))                     # (alpha, gamma): as configured, no alpha, gamma 1

BUILDERS = {}
for _i, (_a, _g) in enumerate(CONFIGS):
    BUILDERS["focal_ladder_a%g_g%g" % (_a, _g)] = functools.partial(_focal_ladder, alpha=_a, gamma=_g, seed=10 + _i)
for _i, (_r, _c) in enumerate(((1, 2), (511, 2), (512, 2), (513, 2), (341, 3), (700, 1), (13, 81), (66000, 2))):
    _a, _g = CONFIGS[_i % 3]
    BUILDERS["focal_%dx%d" % (_r, _c)] = functools.partial(_focal_size, rows=_r, C=_c, alpha=_a, gamma=_g, seed=20 + _i, tail=_r * _c > FOCAL_CAP_CELLS)
FOCAL_LADDER = [k for k in BUILDERS if k.startswith("focal_ladder")]
FOCAL_SIZES = [k for k in BUILDERS if k.startswith("focal_") and k not in FOCAL_LADDER]

RMSE_HW = {7: (1, 7), 1961: (37, 53), 2049: (3, 683), 300: (15, 20), 263000: (500, 526)}
for _i, (_b, _hw) in enumerate([(b, hw) for b in (1, 3, 4, 5) for hw in (7, 1961, 2049)] + [(64, 300), (65, 300), (2, 263000)]):
    BUILDERS["rmse_B%d_HW%d" % (_b, _hw)] = functools.partial(_rmse_case, B=_b, H=RMSE_HW[_hw][0], W=RMSE_HW[_hw][1], seed=40 + _i, edges=_hw >= 300,
                                                              tail=_hw > RMSE_CAP_PIXELS)
RMSE_SHAPES = [k for k in BUILDERS if k.startswith("rmse_B")]
BUILDERS["rmse_on_clamp"] = functools.partial(_rmse_case, B=3, H=15, W=20, seed=60, edges=False, on_clamp=True)
BUILDERS["rmse_no_valid_pixel"] = functools.partial(_rmse_case, B=3, H=15, W=20, seed=61, no_valid=True)
RMSE_ON_CLAMP, RMSE_NO_VALID = "rmse_on_clamp", "rmse_no_valid_pixel"

for _i, (_fh, _fw) in enumerate(((2, 2), (3, 4), (4, 5), (50, 82))):  # HW = 4, 12, 20, 4100: image 1 has no row, image 3 has gsum = 0
    BUILDERS["mask_P9_HW%d" % (_fh * _fw)] = functools.partial(_mask_case, rows=[3, 0, 4, 2], fh=_fh, fw=_fw, seed=70 + _i, gsum0=(3,))
for _i, _p in enumerate((1, 255, 256, 257, 600)):
    BUILDERS["mask_P%d_HW20" % _p] = functools.partial(_mask_case, rows=[0, 1, 0, 0] if _p == 1 else _spread(_p, 4), fh=4, fw=5, seed=80 + _i)
BUILDERS["mask_B64"] = functools.partial(_mask_case, rows=[0 if b in (0, 31, 63) else 1 + b % 3 for b in range(64)], fh=4, fw=5, seed=90, gsum0=(7,))
BUILDERS["mask_saturated"] = functools.partial(_mask_case, rows=[8, 8, 10, 6], fh=12, fw=20, seed=91, saturated=True)
BUILDERS["mask_no_qualifying_image"] = functools.partial(_mask_case, rows=[3, 0, 4, 2], fh=4, fw=5, seed=92, no_qualifying=True)
BUILDERS["mask_dice_only"] = functools.partial(_mask_case, rows=[3, 0, 4, 2], fh=4, fw=5, seed=93, dice_only=True)
MASK_CASES = [k for k in BUILDERS if k.startswith("mask_")]

FOCAL_CASES = FOCAL_LADDER + FOCAL_SIZES
RMSE_CASES = RMSE_SHAPES + [RMSE_ON_CLAMP, RMSE_NO_VALID]
RULES = {"focal": FOCAL_RULES, "rmse": RMSE_RULES, "mask": MASK_RULES}
FAMILY_CASES = {"focal": FOCAL_CASES, "rmse": RMSE_CASES, "mask": MASK_CASES}


@functools.lru_cache(maxsize=None)
def get_case(name):
    return BUILDERS[name](name)
