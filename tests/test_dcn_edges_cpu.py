"""CPU: the inputs of tests/test_dcn_edges_gpu.py really sit on DCNv2's geometric edges, and the bounds used there separate a correct
kernel from the plausible mistakes at those edges.  For EVERY case the GPU file runs (tests/dcn_edge_cases.py):

  class counts       every class of sampling point the case claims holds >= 32 points (-1 and H / W in y and in x separately); the window
                     and CSR cases hold a patch / a bin of every kind they are aimed at; no CSR bin exceeds 256 entries
  mutant separation  the switchable restatement equals oracle/dcn_ref.py to 1e-12 under rule "true", and under every wrong rule that
                     applies to the case at least one of (output, gradients) moves by >= 100 x the bound the GPU test uses for it
  reference in bound the same oracle evaluated in fp32 agrees with fp64 within a tenth of that bound: the reference's own arithmetic is
                     not what the GPU comparison measures"""
import pytest
import torch

import dcn_edge_cases as E

ALL_CASES = list(E.BUILDERS)


def test_case_lists_cover_every_builder():
    assert sorted(E.EDGE_MIX + E.RAW + E.BLOCK + E.WINDOW + E.CSR_SWITCH + E.NARROW + ["csr_convergence"]) == sorted(ALL_CASES)


@pytest.mark.parametrize("name", ALL_CASES)
def test_inputs_are_fp32_exact_on_the_eighth_grid(name):
    c = E.get_case(name)
    for k, v in c.t.items():
        if v is not None:
            assert torch.equal(v.float().double(), v), k
    for k in ("off", "msk", "om"):
        if c.t.get(k) is not None:
            assert torch.equal((c.t[k] * 8).round(), c.t[k] * 8), k
    assert c.max_offset * 8 == round(c.max_offset * 8)
    if c.t.get("msk") is not None:
        assert c.t["msk"].min() >= 0 and c.t["msk"].max() <= 2
    if name.endswith("_mask0"):
        assert int((c.t["msk"] == 0).sum()) >= E.MIN_POINTS
    if name in E.EDGE_MIX + E.CSR_SWITCH:
        assert c.t["off"].abs().max() <= 3.0
        ints = (c.t["off"] == c.t["off"].round()).double().mean().item()
        assert 0.25 <= ints <= 0.45, ints                      # a quarter rounded + the grid's own integers (1/8 of the rest)


@pytest.mark.parametrize("name", ALL_CASES)
def test_claimed_classes_are_populated(name):
    c = E.get_case(name)
    n = c.counts()
    short = {k: n[k] for k in c.claims if n[k] < E.MIN_POINTS}
    assert not short, "%s: classes below %d points: %r (all: %r)" % (name, E.MIN_POINTS, short, n)
    assert int(c.bins().max()) <= E.MAX_BIN, int(c.bins().max())


@pytest.mark.parametrize("name", E.RAW + E.BLOCK)
def test_raw_maps_saturate_the_clamp_and_the_modulator(name):
    c = E.get_case(name)
    om = c.raw_map()
    beyond = (om[:, :18].abs() > c.max_offset).double().mean().item()
    assert beyond >= 0.25, beyond
    if name in E.RAW:
        assert 0.28 <= beyond <= 0.39 and om[:, :18].abs().max() <= 3 * c.max_offset
        assert int((om[:, :18] == c.max_offset).sum()) >= E.MIN_POINTS and int((om[:, :18] == -c.max_offset).sum()) >= E.MIN_POINTS
        for lv in (0.0, 1.0, -1.0, 20.0, -20.0, 100.0, -100.0):
            assert int((om[:, 18:] == lv).sum()) >= E.MIN_POINTS, lv
    # the oracle's reference gradient is exactly zero beyond the clamp and follows torch.clamp at equality
    ref = c.reference()
    if name in E.RAW:
        assert (ref["d_om"][:, :18][om[:, :18].abs() > c.max_offset] == 0).all()
        on = (om[:, :18].abs() == c.max_offset)
        assert float(ref["d_om"][:, :18][on].abs().max()) > 0
        probe = om[:, :18].clone().requires_grad_(True)
        probe.clamp(-c.max_offset, c.max_offset).sum().backward()
        assert (probe.grad[on] == 1).all()                     # torch.clamp passes the gradient at equality: so must the kernel


@pytest.mark.parametrize("name", E.WINDOW)
def test_window_cases_hold_a_patch_of_every_window_class(name):
    c = E.get_case(name)
    box = c.boxes()
    wc = E.window_classes(box, c.H, c.W)
    missing = [k for k in c.patch_claims if int(wc[k].sum()) == 0]
    assert not missing, (missing, box["wh"].tolist(), box["ww"].tolist())
    assert int(((box["wh"] == 33) & (box["ww"] <= E.WPITCH)).sum()) >= 1 and int(((box["ww"] == 41) & (box["wh"] <= E.WROWS)).sum()) >= 1   # each limit alone
    assert int((wc["rows32"] & wc["cols40"]).sum()) >= 1                                   # the largest staged window
    empty = wc["empty"].nonzero()
    assert empty.shape[0] == 1
    y, x = c.coords()
    _, ty, tx = empty[0].tolist()
    sl = (0, slice(None), slice(ty * E.PATCH, (ty + 1) * E.PATCH), slice(tx * E.PATCH, (tx + 1) * E.PATCH))
    assert int(c.classes()["outside"][sl].sum()) == 576


def test_csr_convergence_case_holds_the_bins_it_is_aimed_at():
    c = E.get_case("csr_convergence")
    bins = c.bins()
    assert int(bins.max()) == 256
    for k in range(9):
        assert sorted(bins[0, k][bins[0, k] > 0].tolist()) == [256] * 4                    # image 0: one location per tap, every other bin empty
        assert set(bins[1, k][bins[1, k] > 0].tolist()) == {8, 9}
        assert int((bins[1, k] == 8).sum()) == 60 and int((bins[1, k] == 9).sum()) == 60
    assert c.structural_zeros()["d_x"][0].double().mean() > 0.8


@pytest.mark.parametrize("name,hw", [("csr_hw15360", 15360), ("csr_hw15520", 15520)])
def test_csr_switch_cases_sit_on_either_side_of_the_one_launch_limit(name, hw):
    c = E.get_case(name)
    assert c.H * c.W == hw and (hw <= 15360) == (name == "csr_hw15360")
    bins = c.bins()
    assert int((bins == 8).sum()) > 0 and int((bins >= 9).sum()) > 0                       # both sides of the sorting network


@pytest.mark.parametrize("name", ALL_CASES)
def test_restatement_is_the_oracle_and_every_mutant_is_separated_100x(name):
    c = E.get_case(name)
    ref = c.reference()
    true = c.evaluate(impl="restate", rule="true")
    for k in ref:
        err, den = E.rel_err(true[k], ref[k])
        assert err * den <= 1e-12 * max(1.0, den), (k, err)
    for rule in c.mutants:
        wrong = c.evaluate(impl="restate", rule=rule)
        ratio = {k: E.rel_err(wrong[k], ref[k])[0] / c.bound(k) for k in ref}
        assert max(ratio.values()) >= 100, "%s / %s: largest change is only %.1f x the bound: %r" % (name, rule, max(ratio.values()), ratio)


@pytest.mark.parametrize("name", ALL_CASES)
def test_fp32_oracle_stays_within_a_tenth_of_the_bound(name):
    c = E.get_case(name)
    ref = c.reference()
    f32 = c.evaluate(dtype=torch.float32)
    for k in ref:
        err, _ = E.rel_err(f32[k], ref[k])
        assert err <= 0.1 * c.bound(k), "%s %s: fp32 oracle off by %.2e of the tensor maximum (bound %.1e)" % (name, k, err, c.bound(k))


@pytest.mark.parametrize("name", ALL_CASES)
def test_structural_zeros_are_zero_in_the_reference(name):
    c = E.get_case(name)
    ref = c.reference()
    for k, m in c.structural_zeros().items():
        assert float(ref[k][m].abs().max() if m.any() else 0.0) <= 1e-30 * (1 + float(ref[k].abs().max())), k
