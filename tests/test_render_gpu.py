"""GPU: the overlay, the depth limits and the depth colours drawn on the device (csrc/prn_render.hip through planerecnet_amd.render)
against the host drawing of simple_inference.py (display_on_frame with no_text, _viridis), numpy, and the restatement of the contour
rule (tests/render_restate.py); determinism, no host synchronisation, untouched inputs; simple_inference.py --render device."""
import os

import numpy as np
import pytest
import torch

from render_restate import HAND_MASKS, contour_of, make_case, overlay

pytestmark = pytest.mark.gpu

MAPS = [(5, 7), (3, 1), (8, 12), (33, 64), (96, 128)]              # scalar path (odd widths); wide path: one partial tile, ragged tiles, several tiles
COUNTS = [0, 1, 2, 23]                                             # 23 > 19 colours: the colour table wraps


def _render():
    from planerecnet_amd import render
    return render


def _si():
    import simple_inference as si
    return si


def _result(masks, boxes, device="cuda"):
    m = masks if torch.is_tensor(masks) else torch.from_numpy(masks).to(device)
    n = m.shape[0]
    return {"pred_masks": m, "pred_boxes": torch.from_numpy(boxes), "pred_scores": torch.linspace(0.9, 0.4, n).to(device),
            "pred_depth": torch.ones(1, 1, *m.shape[1:], device=device)}


def _host(frame, masks, boxes, **kw):
    """the oracle: the host drawing on host copies"""
    r = {"pred_masks": torch.from_numpy(np.ascontiguousarray(masks)), "pred_boxes": torch.from_numpy(boxes),
         "pred_scores": torch.linspace(0.9, 0.4, masks.shape[0]), "pred_depth": torch.ones(1, 1, *masks.shape[1:])}
    return torch.from_numpy(np.ascontiguousarray(_si().display_on_frame(r, torch.from_numpy(frame), no_text=True, **kw)[0]))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("H,W", MAPS)
def test_overlay_is_the_host_drawing(H, W, n):
    frame, masks, boxes = make_case(1000 * n + 10 * H + W, n, H, W)
    got = _render().render_overlay(_result(masks, boxes), torch.from_numpy(frame).cuda())
    assert got.dtype == torch.uint8 and got.shape == (H, W, 3) and got.is_cuda
    assert torch.equal(got.cpu(), _host(frame, masks, boxes))
    ref = torch.from_numpy(overlay(frame, masks, boxes, contours=True))
    assert torch.equal(_render().render_overlay(_result(masks, boxes), torch.from_numpy(frame).cuda(), contours=True).cpu(), ref)


def test_overlay_table_chunks():
    frame, masks, boxes = make_case(77, 300, 8, 12)
    f = torch.from_numpy(frame).cuda()
    assert torch.equal(_render().render_overlay(_result(masks, boxes), f).cpu(), _host(frame, masks, boxes))
    assert torch.equal(_render().render_overlay(_result(masks, boxes), f, contours=True).cpu(), torch.from_numpy(overlay(frame, masks, boxes, contours=True)))
    # boxes that do not hide what is below them: every chunk's blend is visible
    assert torch.equal(_render().render_overlay(_result(masks, boxes), f, no_box=True).cpu(), _host(frame, masks, boxes, no_box=True))


@pytest.mark.parametrize("alpha", [0.5, 0.3, 0.77])
@pytest.mark.parametrize("H,W", [(5, 7), (33, 64)])
def test_overlay_alphas_layers_and_mask_kinds(H, W, alpha):
    frame, masks, boxes = make_case(int(alpha * 100) + H, 23, H, W)
    f = torch.from_numpy(frame).cuda()
    ref = _host(frame, masks, boxes, mask_alpha=alpha)
    assert torch.equal(_render().render_overlay(_result(masks, boxes), f, mask_alpha=alpha).cpu(), ref)
    for kw in ({"no_mask": True}, {"no_box": True}):
        assert torch.equal(_render().render_overlay(_result(masks, boxes), f, mask_alpha=alpha, **kw).cpu(), _host(frame, masks, boxes, mask_alpha=alpha, **kw)), kw
        assert torch.equal(_render().render_overlay(_result(masks, boxes), f, mask_alpha=alpha, contours=True, **kw).cpu(),
                           torch.from_numpy(overlay(frame, masks, boxes, alpha=alpha, contours=True, **kw))), kw
    u8 = masks.astype(np.uint8) * np.random.RandomState(3).randint(1, 256, size=masks.shape).astype(np.uint8)      # byte masks: any non-zero value is set
    assert torch.equal(_render().render_overlay(_result(u8, boxes), f, mask_alpha=alpha).cpu(), ref)
    wide = torch.zeros(23, H, 2 * W, dtype=torch.bool, device="cuda")
    wide[:, :, ::2] = torch.from_numpy(masks).cuda()
    view = wide[:, :, ::2]                                           # a non-contiguous view
    assert not view.is_contiguous()
    assert torch.equal(_render().render_overlay(_result(view, boxes), f, mask_alpha=alpha).cpu(), ref)
    shifted = torch.zeros(23 * H * W + 1, dtype=torch.uint8, device="cuda")[1:].view(23, H, W)                        # masks at an odd address: the per-pixel path
    shifted.copy_(torch.from_numpy(u8).cuda())
    assert torch.equal(_render().render_overlay(_result(shifted, boxes), f, mask_alpha=alpha).cpu(), ref)
    assert torch.equal(_render().render_overlay(_result(shifted, boxes), f, mask_alpha=alpha, contours=True).cpu(),
                       torch.from_numpy(overlay(frame, masks, boxes, alpha=alpha, contours=True)))


@pytest.mark.parametrize("name", list(HAND_MASKS))
def test_contours_of_hand_made_masks(name):
    mask, outline = HAND_MASKS[name]
    H, W = mask.shape
    frame = torch.full((H, W, 3), 10.0, device="cuda")
    got = _render().render_overlay(_result(mask[None], np.asarray([[0, 0, 1, 1]], np.float32)), frame, no_mask=True, no_box=True, contours=True).cpu().numpy()
    assert np.array_equal((got == 255).all(-1), outline) and np.array_equal((got == 10).all(-1), ~outline)


def test_crossing_contours():
    H, W = 12, 16
    masks = np.zeros((2, H, W), bool)
    masks[0, 2:9, 1:10] = True
    masks[1, 5:12, 6:15] = True                                      # the outlines cross at (5, 9) and (8, 6)
    both = contour_of(masks[0]) | contour_of(masks[1])
    assert both[5, 9] and both[8, 6] and contour_of(masks[0])[8, 6] and contour_of(masks[1])[8, 6]
    frame, _, _ = make_case(2, 0, H, W)
    boxes = np.asarray([[0, 0, 1, 1], [0, 0, 1, 1]], np.float32)
    got = _render().render_overlay(_result(masks, boxes), torch.from_numpy(frame).cuda(), no_box=True, contours=True).cpu()
    assert torch.equal(got, torch.from_numpy(overlay(frame, masks, boxes, no_box=True, contours=True)))
    assert np.array_equal((got.numpy() == 255).all(-1), both)


def _depth_cases():
    rng = np.random.RandomState(9)
    for n in (1, 2, 101, 4096, 33 * 64):
        d = (rng.randn(n) * 3).astype(np.float32)                   # negative values
        yield "normal-%d" % n, d
        dup = np.round(d).astype(np.float32)                        # duplicates, +0 and -0
        dup[::7] = -0.0
        dup[3::11] = 0.0
        yield "duplicates-%d" % n, dup
        holes = d.copy()
        holes[rng.rand(n) < 0.2] = np.nan
        yield "nan-%d" % n, holes
        yield "all-nan-%d" % n, np.full(n, np.nan, np.float32)


@pytest.mark.parametrize("name,d", list(_depth_cases()), ids=[c[0] for c in _depth_cases()])
def test_depth_limits(name, d):
    lim = _render().depth_limits(torch.from_numpy(d).cuda()).cpu().numpy()
    assert lim.dtype == np.float32 and lim.shape == (8,)
    s = np.sort(d[~np.isnan(d)])
    if s.size == 0:
        assert np.array_equal(lim, np.zeros(8, np.float32))
        return
    want = []
    for q in (1, 99):
        below = int(np.floor((s.size - 1) * (q / 100)))
        want += [s[below], s[min(below + 1, s.size - 1)]]
    assert np.array_equal(lim[2:6], np.asarray(want, np.float32)), (lim, want)
    assert lim[6] == s[0] and lim[7] == s[-1]
    ref = np.nanpercentile(d, [1, 99]).astype(np.float64)
    for got, r in zip(lim[:2].astype(np.float64), ref):
        assert abs(got - r) <= float(np.spacing(np.float32(max(abs(got), abs(r))))), (name, got, r)


def _depth_maps():
    rng = np.random.RandomState(4)
    smooth = (1.5 + np.add.outer(np.linspace(0, 2, 33), np.linspace(0, 1, 64)) + rng.rand(33, 64) * 0.05).astype(np.float32)
    holes = smooth.copy()
    holes[rng.rand(33, 64) < 0.1] = np.nan
    return {"smooth 33x64": smooth, "odd 7x9": smooth[:7, :9].copy(), "constant": np.full((6, 8), 2.5, np.float32), "with NaN": holes,
            "all NaN": np.full((5, 4), np.nan, np.float32), "negative": -smooth[:9, :11].copy()}


@pytest.mark.parametrize("name", list(_depth_maps()))
def test_depth_colours_are_the_host_ramp(name):
    d = _depth_maps()[name]
    dev = torch.from_numpy(d).cuda()
    lim = _render().depth_limits(dev)
    got = _render().colorize_depth(dev[None, None], limits=lim)     # the model's [1,1,H,W]
    assert got.dtype == torch.uint8 and got.shape == d.shape + (3,)
    vmin, vmax = lim.cpu().numpy()[:2]
    with np.errstate(all="ignore"):
        host = _si()._viridis(d, vmin, vmax).astype(np.uint8)       # RGB; what _imwrite_bgr's cast leaves
    assert np.array_equal(got.cpu().numpy()[:, :, ::-1], host)
    assert torch.equal(_render().colorize_depth(dev), got)          # limits computed inside
    if name == "constant":
        assert (got.cpu().numpy() == np.asarray([84, 1, 68], np.uint8)).all()       # level 0, BGR


def test_depth_gray():
    rng = np.random.RandomState(6)
    for shape, shift in (((33, 64), 512.0), ((7, 9), 1000.0)):
        d = (rng.rand(*shape) * (65535 / shift) * 0.999).astype(np.float32)
        got = _render().colorize_depth(torch.from_numpy(d).cuda(), mode="gray", depth_shift=shift)
        assert got.dtype == torch.uint16 and got.shape == shape
        assert np.array_equal(got.cpu().numpy(), (d * shift).astype(np.uint16))
    edge = torch.tensor([[float("nan"), -3.0, 1e9, 2.0]], device="cuda")
    assert _render().colorize_depth(edge, mode="gray", depth_shift=2).cpu().numpy().tolist() == [[0, 0, 65535, 4]]


def test_repeats_are_bit_identical_inputs_untouched_and_no_host_synchronisation():
    frame, masks, boxes = make_case(21, 23, 33, 64)
    f = torch.from_numpy(frame).cuda()
    r = _result(masks, boxes)
    d = torch.from_numpy(_depth_maps()["with NaN"]).cuda()
    keep = {k: v.clone() for k, v in r.items()}
    f0, d0 = f.clone(), d.clone()
    first = (_render().render_overlay(r, f, contours=True), _render().depth_limits(d), _render().colorize_depth(d), _render().colorize_depth(d, mode="gray"))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda").item()                      # the mode does catch a synchronisation
        runs = [(_render().render_overlay(r, f, contours=True), _render().depth_limits(d), _render().colorize_depth(d),
                 _render().colorize_depth(d, mode="gray")) for _ in range(5)]
        plain = _render().render_overlay(r, f)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    for run in runs:
        for a, b in zip(run, first):
            assert torch.equal(a.view(torch.uint8) if a.dtype != torch.float32 else a.view(torch.int32), b.view(torch.uint8) if b.dtype != torch.float32 else b.view(torch.int32))
    assert torch.equal(plain.cpu(), _host(frame, masks, boxes))
    assert set(r) == set(keep)
    for k, v in keep.items():
        assert torch.equal(r[k], v), k
    assert torch.equal(f, f0) and torch.equal(d.view(torch.int32), d0.view(torch.int32))


def test_result_without_detections():
    frame, masks, boxes = make_case(8, 2, 8, 12)
    f = torch.from_numpy(frame).cuda()
    none = {"pred_masks": None, "pred_boxes": None, "pred_classes": None, "pred_scores": None, "pred_depth": torch.ones(1, 1, 8, 12, device="cuda")}
    want = torch.from_numpy(frame.astype(np.uint8))
    assert torch.equal(_render().render_overlay(none, f, contours=True).cpu(), want)
    host, _ = _si().display_on_frame(none, f, no_text=True)
    assert np.array_equal(host, want.numpy())


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """PlaneRecNet_50 with seeded weights whose category bias leaves detections on a small seeded image, and a function that runs
    simple_inference.py's argument parser and its per-image function on that network (the model is built once, not once per flag set)"""
    from PIL import Image
    from oracle import synth
    from planerecnet_amd.config import cfg, set_cfg
    from planerecnet_amd.planerecnet import PlaneRecNet
    si = _si()
    tmp = tmp_path_factory.mktemp("render_cli")
    name = "PlaneRecNet_50_config"
    set_cfg(name)
    rng = np.random.RandomState(5)
    yy, xx = np.mgrid[:96, :128]
    img = np.stack([128 + 100 * np.sin(xx / 9.0 + c) * np.cos(yy / 11.0 - c) for c in (0.0, 1.0, 2.0)], -1)
    src = str(tmp / "frame.png")
    Image.fromarray(np.clip(img + rng.randn(96, 128, 3) * 10, 0, 255).astype(np.uint8)).save(src)
    overrides = {"nms_type": "matrix", "mask_thr": 0.3, "update_thr": 0.3, "top_k": 100}         # what the CLI's defaults put into cfg.solov2
    old = {k: getattr(cfg.solov2, k) for k in overrides}
    old_device, old_args = cfg.device, getattr(si, "args", None)
    cfg.solov2.replace(overrides)
    cfg.device = "cuda:0"
    sd = synth.make_state_dict(name, seed=1)
    net = PlaneRecNet(cfg)

    def run(tag, *flags):
        dst = str(tmp / (tag + ".png"))
        a = si.parse_args(["--image", src + ":" + dst] + list(flags))
        results = si.inference_image(net, src, dst, depth_mode=a.depth_mode)
        return np.asarray(Image.open(dst)), np.asarray(Image.open(str(tmp / (tag + "_dep.png")))), results[0]

    try:
        for shift in (1.0, 2.0, 3.0, 4.0):                          # condition the category bias: detections must survive
            sd_try = dict(sd)
            sd_try["inst_head.cate_pred.bias"] = sd["inst_head.cate_pred.bias"] + shift
            net.load_state_dict(sd_try)
            net = net.cuda().eval()
            probe = run("probe", "--no_text")[2]
            if probe["pred_masks"] is not None and probe["pred_masks"].shape[0] >= 2:
                break
        else:
            raise AssertionError("no bias shift leaves two detections")
        yield run
    finally:
        cfg.solov2.replace(old)
        cfg.device = old_device
        si.args = old_args


def test_cli_device_rendering_is_the_host_rendering(cli):
    from PIL import Image, ImageDraw
    host_seg, host_dep, r = cli("host", "--no_text")
    dev_seg, dev_dep, r2 = cli("device", "--no_text", "--render", "device")
    assert torch.equal(r["pred_masks"], r2["pred_masks"]) and torch.equal(r["pred_depth"], r2["pred_depth"])       # the network repeats itself
    assert host_seg.shape == (480, 640, 3) and np.array_equal(dev_seg, host_seg)
    # the depth picture: equal files where the device limits are numpy's; otherwise compared through the limits read back
    depth = r["pred_depth"].squeeze().float().cpu().numpy()
    lim = _render().depth_limits(r["pred_depth"]).cpu().numpy()
    if lim[0] == np.percentile(depth, 1) and lim[1] == np.percentile(depth, 99):
        assert np.array_equal(dev_dep, host_dep)
    else:
        assert np.array_equal(dev_dep, _si()._viridis(depth, lim[0], lim[1]).astype(np.uint8))
    # with the score texts: equal outside the union of the text extents
    host_txt, _, _ = cli("host_text")
    dev_txt, _, _ = cli("device_text", "--render", "device")
    boxes, scores = r["pred_boxes"].cpu().numpy(), r["pred_scores"].cpu().numpy()
    draw = ImageDraw.Draw(Image.new("RGB", (640, 480)))
    text = np.zeros((480, 640), bool)
    for i in range(scores.shape[0]):
        left, top, right, bottom = draw.textbbox((int(boxes[i][0]) + 2, int(boxes[i][1]) + 2), "plane: %.2f" % scores[i])
        text[max(top, 0):max(bottom, 0), max(left, 0):max(right, 0)] = True
    assert text.any() and not text.all()
    assert np.array_equal(dev_txt[~text], host_txt[~text])
    assert not np.array_equal(dev_txt, dev_seg)                      # texts were drawn
    # --contours changes mask-border pixels only, to white
    cont_seg, _, _ = cli("device_contours", "--no_text", "--render", "device", "--contours")
    masks = r["pred_masks"].cpu().numpy()
    border = np.zeros((480, 640), bool)
    for m in masks:
        border |= contour_of(m != 0)
    changed = (cont_seg != dev_seg).any(-1)
    assert changed.any() and not (changed & ~border).any()
    assert (cont_seg[changed] == 255).all()
    # gray depth mode
    host_gray = cli("host_gray", "--no_text", "--depth_mode", "gray")[1]
    dev_gray = cli("device_gray", "--no_text", "--depth_mode", "gray", "--render", "device")[1]
    assert dev_gray.dtype == host_gray.dtype and np.array_equal(dev_gray, host_gray)
