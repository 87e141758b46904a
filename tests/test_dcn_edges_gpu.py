"""GPU: DCNv2 at its geometric edges against the fp64 oracle (oracle/dcn_ref.py), with the bounds of tests/test_ops_gpu.py: output within
2e-4, gradients within 5e-4 of the tensor maximum.  The inputs (tests/dcn_edge_cases.py) sit on integer positions, exactly on -1 / H / W,
in the border bands, on and beyond the clamp of raw mode, on saturated modulator logits, in every window class of the windowed forward,
in CSR bins of 8 / 9 / 256 entries, on both sides of the one-launch CSR limit and on maps narrower than the pixel pair of the pair-load
table; tests/test_dcn_edges_cpu.py shows that they do and that each plausible mistake there moves a result by >= 100 x these bounds.
Where a gradient is structurally zero it has to be 0.0 bit for bit.  A failure prints the maximum error per class of sampling point.
Every check prints one `dcn-edges` line (case, quantity, error relative to the tensor maximum, bound): profiles/dcn_edges_errors.txt."""
import pytest
import torch

import dcn_edge_cases as E

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def on_gpu(case, grad=True):
    d = dev()
    return {k: case.t[k].float().to(d).requires_grad_(grad) for k in case.leaves}, case.t["go"].float().to(d)


def compare(case, got, names=None):
    """every quantity of `got` against the shared fp64 reference + the exact zeros; one report for all failures"""
    ref = case.reference()
    got = {k: v.detach().double().cpu() for k, v in got.items()}
    bad = []
    for k in (names or got):
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        err, den = E.rel_err(got[k], ref[k])
        print("dcn-edges %-24s %-6s rel %.3e  bound %.1e  (max|ref| %.3e)" % (case.name, k, err, case.bound(k), den))
        if not err <= case.bound(k):                           # (also catches NaN)
            bad.append("%s: max-abs error %.3e of the tensor maximum %.3e, bound %.1e" % (k, err, den, case.bound(k)))
    for k, m in case.structural_zeros().items():
        if k in got and m.any():
            nz = int((got[k][m] != 0).sum())
            print("dcn-edges %-24s %-6s exact zeros: %d of %d entries are not 0.0" % (case.name, k, nz, int(m.sum())))
            if nz:
                bad.append("%s: %d of %d structurally zero entries are not 0.0 (largest %.3e)" % (k, nz, int(m.sum()), got[k][m].abs().max().item()))
    assert not bad, "%s:\n  %s\n  maximum error per class of sampling point (relative to the tensor maximum):\n%s" % (
        case.name, "\n  ".join(bad), E.per_class_report(case, got, ref))


def run_plain(case):
    """ops.deform_conv2d: output and the five gradients"""
    from planerecnet_amd import ops
    t, go = on_gpu(case)
    y = ops.deform_conv2d(t["x"], t["off"], t["w"], t["b"], stride=(case.stride, case.stride), padding=(case.pad, case.pad), mask=t.get("msk"))
    gs = torch.autograd.grad(y, [t[k] for k in case.leaves], go)
    ops.wgrad_join()
    got = {"y": y}
    got.update({"d_" + k: g for k, g in zip(case.leaves, gs)})
    return got, t, go


@pytest.mark.parametrize("name", E.EDGE_MIX)
def test_edge_mix_through_deform_conv2d(name):
    """integer positions, points exactly on -1 / H / W, border bands and outside points on the windowed forward, the gather forward (odd C),
    stride 2 with TM = 2 and TM = 4 with partial tiles; without a mask and with a mask that holds exact zeros"""
    case = E.get_case(name)
    compare(case, run_plain(case)[0])


@pytest.mark.parametrize("name", E.RAW)
def test_raw_mode_primitives(name):
    """raw = 1 through ops.dcn_table / dcn_fwd_raw / dcn_wgrad_raw / dcn_data_grads_raw on an explicit [B, 27, Ho, Wo] map: a third of the
    offsets beyond the clamp (their gradient is exactly 0.0), offsets exactly on +-max_offset (torch.clamp passes the gradient there),
    logits of +-20 / +-100; the inference entry with the ReLU epilogue on the same map"""
    from planerecnet_amd import ops
    case = E.get_case(name)
    t, go = on_gpu(case, grad=False)
    s, mo = case.stride, case.max_offset
    table = ops.dcn_table(t["x"].shape, case.M, t["om"], None, s, 1, 1, mo)
    y = ops.dcn_fwd_raw(t["x"], table, t["w"], t["b"], s, 1, 1, mo)
    dw = ops.dcn_wgrad_raw(t["x"], table, go, case.M, s, 1, 1, mo)
    dx, d_om, _ = ops.dcn_data_grads_raw(t["x"], t["om"], None, t["w"], go, s, 1, 1, mo)
    compare(case, {"y": y, "d_x": dx, "d_om": d_om, "d_w": dw})
    om = case.t["om"]
    on = (om[:, :18].abs() == mo)
    ref_on = case.reference()["d_om"][:, :18][on]
    got_on = d_om.cpu().double()[:, :18][on]
    assert (got_on - ref_on).abs().max().item() <= E.GRAD_RTOL * case.reference()["d_om"].abs().max().item()
    assert int((got_on != 0).sum()) >= int((ref_on.abs() > 1e-3 * ref_on.abs().max()).sum()) > 0      # gradient passed at equality, as torch.clamp does
    with torch.no_grad():
        yr = ops.deform_conv2d_raw_relu(t["x"], t["om"], t["w"], t["b"], s, mo)
    ref = case.reference()["y"].clamp(min=0)
    err, den = E.rel_err(yr.double().cpu(), ref)
    print("dcn-edges %-24s %-6s rel %.3e  bound %.1e  (max|ref| %.3e)" % (case.name, "relu_y", err, E.FWD_RTOL, den))
    assert err <= E.FWD_RTOL, ("raw relu forward", err)
    assert bool((yr >= 0).all())


@pytest.mark.parametrize("name", E.BLOCK)
def test_raw_mode_whole_node(name):
    """ops.deform_conv_block with offset biases that saturate the clamp (>= 25 % of the offsets of the reference's own map) and saturated
    modulator logits: output and the gradients of x, w27, b27, w and b"""
    from planerecnet_amd import ops
    case = E.get_case(name)
    om = case.raw_map()
    assert (om[:, :18].abs() > case.max_offset).double().mean().item() >= 0.25
    t, go = on_gpu(case, grad=False)
    w27, b27 = t["w27"], t["b27"]
    leaves = [t["x"].requires_grad_(True), w27[:18].requires_grad_(True), w27[18:].requires_grad_(True), b27[:18].requires_grad_(True),
              b27[18:].requires_grad_(True), t["w"].requires_grad_(True), t["b"].requires_grad_(True)]
    y = ops.deform_conv_block(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], w27, b27, leaves[5], leaves[6], case.stride, case.max_offset)
    g = torch.autograd.grad(y, leaves, go)
    ops.wgrad_join()
    compare(case, {"y": y, "d_x": g[0], "d_w27": torch.cat([g[1], g[2]]), "d_b27": torch.cat([g[3], g[4]]), "d_w": g[5], "d_b": g[6]})


@pytest.mark.parametrize("name", E.WINDOW)
def test_window_classes_of_the_windowed_forward(name):
    """one 8 x 8 patch per class: no live point at all, windows of <= 256 / <= 512 / more elements, exactly 32 rows / 40 columns (staged),
    33 rows / 41 columns (fallback), windows reaching row / column -1 and H / W.  The gradients run the pair-load table and make_tap on
    the same data."""
    case = E.get_case(name)
    compare(case, run_plain(case)[0])


def test_csr_bins_of_8_9_and_256_entries_and_run_to_run_equality():
    """input gradient: bins on both sides of the sorting network's limit (8 / 9), bins shared by all 256 points of a tap plane, empty bins
    (dx exactly 0.0); three runs give one result"""
    case = E.get_case("csr_convergence")
    got, t, go = run_plain(case)
    compare(case, got)
    from planerecnet_amd import ops
    for rep in range(2):
        y = ops.deform_conv2d(t["x"], t["off"], t["w"], t["b"], stride=(1, 1), padding=(1, 1), mask=t["msk"])
        gx, = torch.autograd.grad(y, [t["x"]], go)
        assert torch.equal(gx, got["d_x"]), "dx differs in repetition %d: %g" % (rep + 1, (gx - got["d_x"]).abs().max().item())


@pytest.mark.parametrize("name", E.CSR_SWITCH)
def test_csr_construction_on_either_side_of_15360_bins(name):
    """H * W = 15360: the last one-launch CSR build (a tap plane's bins in LDS); 97 x 160: the first five-launch build; edge-mix offsets"""
    case = E.get_case(name)
    compare(case, run_plain(case)[0])


@pytest.mark.parametrize("name", E.NARROW)
def test_narrow_maps(name):
    """W of 1 and 2 (the pair-load table clamps its pair to column W - 2) and H of 1 and 2: computed, and equal to the oracle"""
    case = E.get_case(name)
    compare(case, run_plain(case)[0])
