"""CPU: the inputs of tests/test_loss_edges_gpu.py really sit on the saturated, boundary and launch-shape edges of the fused loss kernels
(csrc/prn_loss.hip), and the bounds used there separate a correct kernel from the plausible mistakes at those edges.  For EVERY case the GPU
file runs (tests/loss_edge_cases.py):

  inputs             are numbers fp32 holds exactly
  class counts       every element class the case claims holds >= MIN_CELLS elements (the focal ladder: per rung x sign x cell kind, half of
                     them in each class); every shape case enters the branch it is aimed at, computed from the kernels' launch constants,
                     which are restated here as numbers next to the kernel line they come from
  restatement        the switchable restatement under rule "true" equals the plain fp64 operator chain of losses.py to 1e-12
  mistakes           under every wrong rule, on at least one case it applies to, a checked quantity moves by >= 100 x the bound the GPU test
                     uses for it, under the GPU test's own metric (per-image / per-row scales and the row floor included)
  reference in bound the plain operator chain evaluated in fp32 on the CPU agrees with fp64 within a QUARTER of that bound"""
import math

import pytest
import torch

import loss_edge_cases as E

ALL_CASES = list(E.BUILDERS)
FINITE_CASES = [n for n in ALL_CASES if n != E.RMSE_NO_VALID]


def cdiv(a, b):
    return (a + b - 1) // b


def test_case_lists_cover_every_builder():
    assert sorted(E.FOCAL_CASES + E.RMSE_CASES + E.MASK_CASES) == sorted(ALL_CASES)
    assert E.MIN_CELLS >= 8 and E.BOUND == 1e-5


@pytest.mark.parametrize("name", ALL_CASES)
def test_inputs_are_fp32_exact(name):
    c = E.get_case(name)
    for k, v in c.t.items():
        if v is not None and v.dtype.is_floating_point:
            assert v.dtype == torch.float64 and torch.equal(v.float().double(), v), k
    assert E.MIN_DEPTH == float(torch.tensor(E.MIN_DEPTH).float()) and E.CLAMP == float(torch.tensor(E.CLAMP).float())
    assert E.MIN_DEPTH < E.NEXT_ABOVE_MIN_DEPTH < E.MIN_DEPTH * (1 + 2e-7)


@pytest.mark.parametrize("name", ALL_CASES)
def test_claimed_classes_are_populated(name):
    c = E.get_case(name)
    n = c.counts()
    short = {k: (n[k], m) for k, m in c.claims.items() if n[k] < m}
    assert not short, "%s: classes below their minimum (count, minimum): %r" % (name, short)


# ------------------------------------------------------------------------------------------------ focal: ladder and launch shapes
@pytest.mark.parametrize("name", E.FOCAL_LADDER)
def test_focal_ladder_holds_every_rung_on_both_signs_classes_and_cell_kinds(name):
    c = E.get_case(name)
    assert len(c.claims) == len(E.LADDER) * 2 * 2 * 3                                      # rung x sign x kind x (all, class 0, class 1)
    assert all(m >= (E.MIN_CELLS if ":class" not in k else E.MIN_CELLS // 2) for k, m in c.claims.items())
    cells = c.par["rows"] * c.par["C"]
    assert cdiv(cells, 1024) == 1                      # prn_focal_sum_fwd: nb = cdiv(n, 256 * 4) -- one reduction block
    dead = E.focal_dead_cells(c.t["x"], c.t["labels"])
    ref = c.reference()["d_x"]
    assert int(dead.sum()) >= (12 + 4) * E.MIN_CELLS    # the cells a gradient formed through p_t loses: negative x >= 17.5 (12 rungs), positive x <= -89 (4 rungs) ...
    assert float(ref[dead].abs().min()) >= 0.25 * E.GO_FOCAL * 0.999                     # ... carry the largest ones: alpha resp. 1 - alpha resp. 1
    assert bool(torch.isfinite(ref).all())


@pytest.mark.parametrize("name", E.FOCAL_SIZES)
def test_focal_size_cases_enter_the_branch_they_aim_at(name):
    c = E.get_case(name)
    rows, C = c.par["rows"], c.par["C"]
    n, cnt = rows * C, c.counts()
    blocks = cdiv(n, 1024)                             # prn_focal_sum_fwd: nb = cdiv(n, 256 * 4), capped at RED_BLOCKS = 128
    expect = {"focal_1x2": 1, "focal_511x2": 1, "focal_512x2": 1, "focal_513x2": 2, "focal_341x3": 1, "focal_700x1": 1, "focal_13x81": 2, "focal_66000x2": 129}
    assert blocks == expect[name]
    assert (blocks > 128) == (name == "focal_66000x2") == (n > E.FOCAL_CAP_CELLS) and E.FOCAL_CAP_CELLS == 128 * 1024
    assert n % 256 != 0 or name == "focal_512x2"       # prn_focal_sum_bwd: cdiv(n, 256) blocks, a partial last one except at 512 x 2
    assert cnt["first_row_positive"] == 1 and cnt["last_class_positives"] >= 1
    if n > E.FOCAL_CAP_CELLS:
        assert cnt["tail_wrong_side"] == 3 and n - E.FOCAL_CAP_CELLS >= 3
    else:
        assert cnt["last_row_positive"] == 1
    if C > 1:
        assert cnt["background_rows"] >= 1 or rows == 1
    assert int((c.t["labels"] > C).sum()) == 0 and int((c.t["labels"] < 0).sum()) == 0


# ------------------------------------------------------------------------------------------------ RMSE-log: launch shapes and value edges
@pytest.mark.parametrize("name", E.RMSE_CASES)
def test_rmse_cases_enter_the_branch_they_aim_at(name):
    c = E.get_case(name)
    B, HW = c.par["B"], c.par["H"] * c.par["W"]
    assert tuple(c.t["pred"].shape) == (B, HW)
    blocks = cdiv(HW, 2048)                            # prn_rmse_log_fwd: nb = cdiv(HW, 256 * 8), capped at RED_BLOCKS = 128
    assert blocks == {7: 1, 1961: 1, 2049: 2, 300: 1, 263000: 129}[HW]
    assert (blocks > 128) == (HW > E.RMSE_CAP_PIXELS) and E.RMSE_CAP_PIXELS == 128 * 2048
    serial = B > 64                                    # rmse_log_final_kernel: `if (B > 64)` -- no LDS slot per image, the one-thread form
    assert serial == (name == "rmse_B65_HW300")
    valid = c.counts()["valid_per_image"]
    if name == E.RMSE_NO_VALID:
        assert valid[1] == 0 and min(valid[0], valid[2]) > 1
        return
    assert min(valid) >= 1
    if B >= 3:
        assert valid[1] == 1 and len(set(valid)) >= min(B, 3) - (1 if HW == 7 else 0)      # counts differ per image, one image has exactly one valid pixel
        ratio = (c.t["pred"][B - 1] / c.t["gt"][B - 1])[c.t["gt"][B - 1] > E.MIN_DEPTH]
        assert float((ratio / 1e4 - 1).abs().max()) < 1e-6
    if HW > E.RMSE_CAP_PIXELS:
        tail = c.t["gt"][:, E.RMSE_CAP_PIXELS:] > E.MIN_DEPTH
        assert bool(tail.all()) and tail.shape[1] == HW - E.RMSE_CAP_PIXELS
    if name == E.RMSE_ON_CLAMP:
        assert c.counts()["pred_on_clamp"] >= E.MIN_CELLS
        on = (c.t["pred"] == E.CLAMP) & (c.t["gt"] > E.MIN_DEPTH)
        g = c.reference()["d_pred"]
        assert float(g[on].abs().min()) > 1e6 * float(g[1:].abs().max())                   # ~1e9 x the others: why the case stands alone
        probe = c.t["pred"].clone().requires_grad_(True)
        probe.clamp(min=E.CLAMP).sum().backward()
        assert bool((probe.grad[on] == 1).all())                                          # torch.clamp passes the gradient at equality: so must the kernel


def test_rmse_shape_cases_cover_the_wave_loop_of_the_final_kernel():
    Bs = sorted({E.get_case(n).par["B"] for n in E.RMSE_SHAPES})
    assert Bs == [1, 2, 3, 4, 5, 64, 65]               # rmse_log_final_kernel: `for (b = wave; b < B; b += 4)` -- B % 4 in {1, 2, 3, 0}, B = 64 the last LDS slot
    assert {b % 4 for b in Bs if b <= 64} == {0, 1, 2, 3}
    for n in E.RMSE_SHAPES:
        c = E.get_case(n)
        want = {"gt_on_min_depth", "gt_next_above_min_depth", "gt_zero", "pred_zero", "pred_negative", "pred_tiny"} if c.par["H"] * c.par["W"] >= 300 else set()
        assert set(c.claims) == want, n


# ------------------------------------------------------------------------------------------------ mask loss: launch shapes and row kinds
@pytest.mark.parametrize("name", E.MASK_CASES)
def test_mask_cases_enter_the_branch_they_aim_at(name):
    c = E.get_case(name)
    P, B, HW = c.par["P"], c.par["B"], c.par["HW"]
    cnt = c.counts()
    assert HW % 4 == 0 and B <= 64 and P == sum(cnt["rows_per_image"])                      # prn_mask_loss_fwd's preconditions
    img = c.t["img"]
    assert bool((img[1:] >= img[:-1]).all()) and torch.equal(torch.bincount(img, minlength=B), torch.tensor(cnt["rows_per_image"]))    # image by image
    hw4 = HW // 4
    empty_splits = sum(1 for s in range(4) if hw4 * s // 4 == hw4 * (s + 1) // 4)           # mask_loss_partial_kernel: ML_SPLITS = 4, beg = HW4 * s / 4
    grid_y = max(1, cdiv(hw4, 1024))                   # prn_mask_loss_bwd: gy = cdiv(HW / 4, 256 * 4)
    strided = P > 256                                  # mask_loss_final_kernel: `for (i = threadIdx.x; i < P; i += 256)` runs more than once
    expect = {"mask_P9_HW4": (3, 1, False), "mask_P9_HW12": (1, 1, False), "mask_P9_HW20": (0, 1, False), "mask_P9_HW4100": (0, 2, False),
              "mask_P1_HW20": (0, 1, False), "mask_P255_HW20": (0, 1, False), "mask_P256_HW20": (0, 1, False), "mask_P257_HW20": (0, 1, True),
              "mask_P600_HW20": (0, 1, True)}
    if name in expect:
        assert (empty_splits, grid_y, strided) == expect[name]
        assert P == int(name.split("_")[1][1:]) and HW == int(name.split("HW")[1])
    if name.startswith("mask_P9_HW"):
        assert cnt["images_npos0"] == 1 and cnt["images_gsum0"] == 1 and cnt["qualifying_images"] == 2
    if name == "mask_B64":
        assert B == 64 and [b for b, r in enumerate(cnt["rows_per_image"]) if r == 0] == [0, 31, 63]
    if name == "mask_no_qualifying_image":
        assert cnt["qualifying_images"] == 0 and float(c.t["adj"].abs().min()) > 0
        ref = c.reference()
        assert float(ref["lav"]) == 0.0
        z = c.t["z"].clone().requires_grad_(True)
        lav = E.mask_restated(z, c.t["labels"], c.t["img"], c.t["adj"], c.t["gsum"], c.t["npos"], E.W_INS, E.W_LAV)[1]
        assert float(torch.autograd.grad(lav, z)[0].abs().max()) == 0.0
    if name == "mask_dice_only":
        assert c.t["adj"] is None and float(c.reference()["lav"]) == 0.0
    if name == "mask_saturated":
        assert HW == 240 and cnt["target_pixels_of_wrong_rows_above_-20"] == 0
        t, z = c.t["labels"], c.t["z"]
        kinds = torch.arange(P) % 4
        assert int(t[kinds == 2].sum()) == 0 and int((t[kinds == 3] == 0).sum()) == 0
        assert int(t[kinds == 1].sum(1).min()) >= E.MIN_CELLS                             # confidently wrong rows do have target pixels
        sat = z.abs() >= 20
        right = ((z > 0) == (t == 1))
        assert bool(right[sat & (kinds != 1).view(-1, 1)].all()) and not bool(right[sat & (kinds == 1).view(-1, 1)].any())


# ------------------------------------------------------------------------------------------------ restatement, mistakes, fp32 chain
@pytest.mark.parametrize("name", ALL_CASES)
def test_restatement_under_rule_true_is_the_plain_fp64_operator_chain(name):
    c = E.get_case(name)
    ref, plain = c.reference(), c.evaluate(impl="plain")
    if c.nan_value:
        assert math.isnan(float(ref["value"])) and math.isnan(float(plain["value"]))
        return
    assert set(ref) == set(c.quantities())
    for k in ref:
        assert bool(torch.isfinite(ref[k]).all()), k
        den = float(ref[k].abs().max())
        assert float((plain[k] - ref[k]).abs().max()) <= 1e-12 * max(1.0, den), (k, float((plain[k] - ref[k]).abs().max()), den)


@pytest.mark.parametrize("family,rule", [(f, r) for f in ("focal", "rmse", "mask") for r in E.RULES[f]])
def test_every_mistake_is_separated_100x_under_the_gpu_metric(family, rule):
    best, where = 0.0, None
    applies = [n for n in E.FAMILY_CASES[family] if rule in E.get_case(n).rules()]
    assert applies, "no case for rule %s" % rule
    for n in applies:
        c = E.get_case(n)
        ref, wrong = c.reference(), c.reference(rule=rule)
        for k in c.quantities():
            err = c.metric(k, wrong[k], ref[k])[0]
            ratio = err / c.bound(k) if err == err else float("inf")
            if ratio > best:
                best, where = ratio, (n, k)
    print("loss-edges separated %-6s %-26s %.3g x the bound on %s %s (%d cases)" % (family, rule, best, where[0], where[1], len(applies)))
    assert best >= 100, "%s / %s: the largest change over %r is only %.1f x the bound" % (family, rule, applies, best)


def test_the_parents_two_mistakes_are_among_the_separated_rules():
    assert "grad_vanishes_at_pt0" in E.FOCAL_RULES and "strict_clamp_grad" in E.RMSE_RULES
    for n in E.FOCAL_LADDER:
        assert "grad_vanishes_at_pt0" in E.get_case(n).rules()
    assert "strict_clamp_grad" in E.get_case(E.RMSE_ON_CLAMP).rules()


@pytest.mark.parametrize("name", FINITE_CASES)
def test_fp32_operator_chain_stays_within_a_quarter_of_the_bound(name):
    c = E.get_case(name)
    ref, f32 = c.reference(), c.evaluate(dtype=torch.float32, impl="plain")
    for k in c.quantities():
        err, scale = c.metric(k, f32[k], ref[k])
        print("loss-edges fp32-chain %-28s %-8s rel %.3e  quarter %.2e  (scale %.3e)" % (name, k, err, 0.25 * c.bound(k), scale))
        assert err <= 0.25 * c.bound(k), "%s %s: the fp32 operator chain is off by %.2e (bound %.1e)" % (name, k, err, c.bound(k))


@pytest.mark.parametrize("name", FINITE_CASES)
def test_structural_zeros_are_zero_in_the_reference(name):
    c = E.get_case(name)
    ref = c.reference()
    for k, m in c.structural_zeros().items():
        assert m.shape == ref[k].shape
        if m.any():
            assert float(ref[k][m].abs().max()) == 0.0, k
    if c.family == "rmse":
        live = ~c.structural_zeros()["d_pred"]
        assert int(live.sum()) > 0 and int((ref["d_pred"][live] == 0).sum()) == 0          # ... and nowhere else
