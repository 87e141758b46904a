"""GPU: the fused loss kernels (csrc/prn_loss.hip: prn_focal_sum_*, prn_rmse_log_*, prn_mask_loss_*) through their autograd functions
(losses._FocalSum, _RmseLog, _MaskLoss) against the fp64 reference of tests/loss_edge_cases.py, with the project's bound for these kernels
(1e-5, tests/test_model_gpu.py and tests/test_ops_gpu.py): scalars |got - ref| <= 1e-5 |ref|; gradients max-abs error <= 1e-5 of the tensor
maximum (focal), of each image's maximum (RMSE-log), per row of max(row maximum, 1e-4 x tensor maximum) (mask loss).  The inputs sit on
saturated logits of both signs on positive and negative cells, on and next to min_depth, on and below the clamp, on either side of every
launch-shape branch (one / two / capped reduction blocks, B = 64 / 65, empty splits, P around 256, two backward blocks per row) and on the
qualification rules of the lava term; tests/test_loss_edges_cpu.py shows that they do and that each plausible mistake there moves a result by
>= 100 x these bounds.  Where a gradient is structurally zero it has to be 0.0 bit for bit.
Every check prints one `loss-edges` line (case, quantity, relative error, bound, scale): profiles/loss_edges_errors.txt."""
import math

import pytest
import torch

import loss_edge_cases as E

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def up(v):
    return None if v is None else (v.float() if v.dtype.is_floating_point else v).to(dev())


def compare(case, got):
    """every quantity of `got` against the shared fp64 reference + the exact zeros; one report for all failures"""
    ref = case.reference()
    got = {k: v.detach().double().cpu().reshape(ref[k].shape) for k, v in got.items()}
    bad = []
    for k in case.quantities():
        err, scale = case.metric(k, got[k], ref[k])
        print("loss-edges %-28s %-8s rel %.3e  bound %.1e  (scale %.3e)" % (case.name, k, err, case.bound(k), scale))
        if not err <= case.bound(k):                           # (also catches NaN)
            bad.append("%s: error %.3e of the scale %.3e, bound %.1e" % (k, err, scale, case.bound(k)))
    for k, m in case.structural_zeros().items():
        if m.any():
            nz = int((got[k][m] != 0).sum())
            print("loss-edges %-28s %-8s exact zeros: %d of %d entries are not 0.0" % (case.name, k, nz, int(m.sum())))
            if nz:
                bad.append("%s: %d of %d structurally zero entries are not 0.0 (largest %.3e)" % (k, nz, int(m.sum()), got[k][m].abs().max().item()))
    assert not bad, "%s:\n  %s" % (case.name, "\n  ".join(bad))


def run_focal(name):
    from planerecnet_amd.losses import _FocalSum
    case = E.get_case(name)
    x = up(case.t["x"]).requires_grad_(True)
    value = _FocalSum.apply(x, up(case.t["labels"]), case.par["alpha"], case.par["gamma"])
    gx, = torch.autograd.grad(value * E.GO_FOCAL, x)
    compare(case, {"value": value, "d_x": gx})


@pytest.mark.parametrize("name", E.FOCAL_LADDER)
def test_focal_saturation_ladder(name):
    """logits of magnitude 0 .. 120 of both signs on positive and on negative cells of both classes, one reduction block: where fp32 p_t
    rounds to 0 (negative cell, x >= 16.7; positive cell, x <= -88.7) the gradient is alpha / 1 - alpha / 1, the largest of the tensor"""
    run_focal(name)


@pytest.mark.parametrize("name", E.FOCAL_SIZES)
def test_focal_sizes(name):
    """one cell pair, either side of one / two reduction blocks, C = 3 / 1 / 81 (the i / C and i % C arithmetic), past the 128-block cap"""
    run_focal(name)


def run_rmse(case):
    from planerecnet_amd.losses import _RmseLog
    B, H, W = case.par["B"], case.par["H"], case.par["W"]
    pred = up(case.t["pred"]).view(B, 1, H, W).requires_grad_(True)
    value = _RmseLog.apply(pred, up(case.t["gt"]).view(B, 1, H, W), E.MIN_DEPTH, E.CLAMP)
    return value, pred


@pytest.mark.parametrize("name", E.RMSE_SHAPES + [E.RMSE_ON_CLAMP])
def test_rmse_log_shapes_and_value_edges(name):
    """B = 1 .. 5, 64 (the last LDS slot) and 65 (the serial form), one / two / capped reduction blocks per image; ground truth on, next above
    and below min_depth, predictions 0 / negative / 1e-30 (value from log(clamp), gradient exactly 0.0), one image with a single valid pixel, one
    with pred / gt = 1e4; rmse_on_clamp: predictions exactly on the clamp, where torch.clamp passes the gradient"""
    case = E.get_case(name)
    value, pred = run_rmse(case)
    gp, = torch.autograd.grad(value * E.GO_RMSE, pred)
    compare(case, {"value": value, "d_pred": gp})


def test_rmse_log_image_without_a_valid_pixel_gives_nan():
    """0 / 0 like the operator chain"""
    case = E.get_case(E.RMSE_NO_VALID)
    assert math.isnan(float(case.reference()["value"]))
    value, _ = run_rmse(case)
    print("loss-edges %-28s %-8s got %r  (reference nan)" % (case.name, "value", float(value)))
    assert math.isnan(float(value))


@pytest.mark.parametrize("name", E.MASK_CASES)
def test_mask_loss_shapes_saturation_and_qualification(name):
    """HW / 4 of 1, 3 (empty splits), 5 and 1025 (two backward blocks per row); P of 1, 255, 256, 257 and 600 (the stride loop and tree of the
    final kernel); 64 images of which three own no row; rows of +-20 .. +-120 logits that are confidently right, confidently wrong, have an empty
    or an all-ones target; images with gsum = 0 or without rows, no qualifying image at all (lav and its gradient exactly 0.0), Dice only"""
    from planerecnet_amd.losses import _MaskLoss
    case = E.get_case(name)
    t, p = case.t, case.par
    z = up(t["z"]).view(p["P"], p["fh"], p["fw"]).requires_grad_(True)
    adj = None if t["adj"] is None else up(t["adj"]).view(p["B"], 1, p["fh"], p["fw"])
    ins, lav = _MaskLoss.apply(z, up(t["labels"]).view(p["P"], p["fh"], p["fw"]), up(t["img"]), adj, up(t["gsum"]), up(t["npos"]), E.W_INS, E.W_LAV)
    gz, = torch.autograd.grad(E.GO_MASK[0] * ins + E.GO_MASK[1] * lav, z, retain_graph=True)
    compare(case, {"ins": ins, "lav": lav, "d_logits": gz})
    if case.counts()["qualifying_images"] == 0:
        gl, = torch.autograd.grad(lav, z)
        nz = int((gl != 0).sum())
        print("loss-edges %-28s %-8s exact zeros: %d of %d entries are not 0.0" % (case.name, "d_lav", nz, gl.numel()))
        assert float(lav) == 0.0 and nz == 0, (float(lav), nz)
