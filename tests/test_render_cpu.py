"""CPU: the host side of the device drawing (planerecnet_amd.render, csrc/prn_render.hip): refusals before any launch, the colour
table against simple_inference._viridis, the numpy restatement of the overlay (tests/render_restate.py) against the host drawing
simple_inference.display_on_frame, and its contour rule on hand-made masks."""
import ctypes

import numpy as np
import pytest
import torch

from render_restate import HAND_MASKS, contour_of, make_case, overlay


def _result(masks, boxes):
    n = masks.shape[0]
    return {"pred_masks": torch.from_numpy(masks), "pred_boxes": torch.from_numpy(boxes), "pred_scores": torch.linspace(0.9, 0.4, n),
            "pred_depth": torch.ones(1, 1, *masks.shape[1:])}


def test_entry_points_validate_before_any_launch():
    from planerecnet_amd import _lib
    lib = _lib.lib
    err = lambda: lib.prn_last_error().decode()      # noqa: E731
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)             # (never dereferenced: validation precedes the launch)
    for N, H, W in ((1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, 65536, 65536)):
        assert lib.prn_render_overlay(p, p, p, p, N, H, W, 0.5, 0.5, 7, q, None) != 0 and "bad sizes" in err(), (N, H, W)
    assert lib.prn_render_overlay(p, p, p, p, 1, 8, 8, 0.5, 0.5, 8, q, None) != 0 and "layer" in err()
    assert lib.prn_render_overlay(None, p, p, p, 1, 8, 8, 0.5, 0.5, 7, q, None) != 0 and "null frame" in err()
    assert lib.prn_render_overlay(p, p, p, p, 1, 8, 8, 0.5, 0.5, 7, p, None) != 0 and "alias" in err()
    assert lib.prn_render_overlay(p, None, p, p, 1, 8, 8, 0.5, 0.5, 1, q, None) != 0 and "null masks" in err()
    assert lib.prn_render_overlay(p, p, None, p, 1, 8, 8, 0.5, 0.5, 4, q, None) != 0 and "colour" in err()
    assert lib.prn_render_overlay(p, p, p, None, 1, 8, 8, 0.5, 0.5, 4, q, None) != 0 and "null boxes" in err()
    assert lib.prn_render_limits_ws_bytes() == 4 * 6 * 256 * 4
    assert lib.prn_render_depth_limits(p, 0, 0.01, 0.99, p, p, None) != 0 and "bad size" in err()
    assert lib.prn_render_depth_limits(p, 1 << 31, 0.01, 0.99, p, p, None) != 0 and "bad size" in err()
    assert lib.prn_render_depth_limits(p, 8, -0.1, 0.99, p, p, None) != 0 and "quantiles" in err()
    assert lib.prn_render_depth_limits(p, 8, 0.01, 0.99, p, None, None) != 0 and "null" in err()
    assert lib.prn_render_depth_limits(p, 8, 0.01, 0.99, p, ctypes.c_void_p(4100), None) != 0 and "aligned" in err()
    assert lib.prn_render_depth_colors(p, 0, p, p, p, None) != 0 and "bad size" in err()
    assert lib.prn_render_depth_colors(p, 8, None, p, p, None) != 0 and "null" in err()
    assert lib.prn_render_depth_gray(p, 8, 512.0, None, None) != 0 and "null" in err()
    assert lib.prn_render_depth_gray(p, 8, 512.0, ctypes.c_void_p(4097), None) != 0 and "aligned" in err()


def test_render_api_refuses_wrong_inputs():
    from planerecnet_amd import render
    frame, masks, boxes = make_case(0, 3, 6, 8)
    ok = _result(masks, boxes)
    f = torch.from_numpy(frame)
    with pytest.raises(RuntimeError, match=r"frame must be a \[H,W,3\] fp32"):
        render.render_overlay(ok, f.double())
    with pytest.raises(RuntimeError, match=r"frame must be a \[H,W,3\] fp32"):
        render.render_overlay(ok, f.permute(2, 0, 1))
    with pytest.raises(RuntimeError, match=r"frame must be a \[H,W,3\] fp32"):
        render.render_overlay(ok, frame)                            # an array, not a tensor
    for shape in ((0, 8, 3), (6, 0, 3)):
        with pytest.raises(RuntimeError, match="must not be empty"):
            render.render_overlay(ok, torch.zeros(shape))
    with pytest.raises(RuntimeError, match="pred_masks must be a bool / uint8"):
        render.render_overlay(dict(ok, pred_masks=ok["pred_masks"].float()), f)
    with pytest.raises(RuntimeError, match="pred_masks must be a bool / uint8"):
        render.render_overlay(dict(ok, pred_masks=ok["pred_masks"][:, :5]), f)
    with pytest.raises(RuntimeError, match=r"pred_boxes must be \[3,4\]"):
        render.render_overlay(dict(ok, pred_boxes=ok["pred_boxes"][:2]), f)
    with pytest.raises(RuntimeError, match="pred_boxes must be a host tensor"):
        render.render_overlay(dict(ok, pred_boxes=boxes), f)
    with pytest.raises(RuntimeError, match="device tensor"):        # everything else is in order: only the device is missing
        render.render_overlay(ok, f)
    with pytest.raises(RuntimeError, match="depth must be a fp32 device tensor"):
        render.depth_limits(torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="between 1 and"):
        render.depth_limits(torch.zeros(0, 4))
    with pytest.raises(RuntimeError, match="device tensor"):
        render.depth_limits(torch.zeros(4, 4))
    with pytest.raises(ValueError, match="two percentages"):
        render.depth_limits(torch.zeros(4, 4), q=(1, 101))
    with pytest.raises(ValueError, match="mode must be"):
        render.colorize_depth(torch.zeros(4, 4), mode="jet")
    with pytest.raises(RuntimeError, match=r"one \[H,W\] map"):
        render.colorize_depth(torch.zeros(2, 4, 4))


def test_reversed_boxes_are_refused_like_pillow():
    from PIL import Image, ImageDraw
    from planerecnet_amd import render
    frame, masks, boxes = make_case(1, 2, 6, 8)
    f = torch.from_numpy(frame)
    for bad, what in (([5.0, 1.0, 2.0, 4.0], "x1 must be greater than or equal to x0"), ([1.0, 4.0, 5.0, 2.0], "y1 must be greater than or equal to y0")):
        b = boxes.copy()
        b[1] = bad
        with pytest.raises(ValueError, match=what):
            render.render_overlay(_result(masks, b), f)
        with pytest.raises(ValueError, match=what):                 # Pillow's own words
            ImageDraw.Draw(Image.new("RGB", (8, 6))).rectangle([int(v) for v in bad], outline=(1, 2, 3), width=1)
        with pytest.raises(RuntimeError, match="device tensor"):    # boxes that are not drawn are not checked (as on the host)
            render.render_overlay(_result(masks, b), f, no_box=True)
    assert render.box_table(torch.tensor([[1.9, -0.5, 2.2, 7.99]]), 1) == [[1, 0, 2, 7]]


def test_cli_refuses_contours_without_device_rendering(capsys):
    import simple_inference as si
    with pytest.raises(SystemExit):
        si.parse_args(["--image", "a.png", "--contours"])
    assert "--contours needs --render device" in capsys.readouterr().err
    a = si.parse_args(["--image", "a.png", "--render", "device", "--contours"])
    assert a.render == "device" and a.contours
    a = si.parse_args(["--image", "a.png"])
    assert a.render == "host" and not a.contours
    with pytest.raises(SystemExit):
        si.parse_args(["--image", "a.png", "--render", "gpu"])
    capsys.readouterr()


def test_colour_table_is_the_host_ramp_on_all_levels():
    import simple_inference as si
    from planerecnet_amd import render
    depth = np.arange(256, dtype=np.float32).reshape(16, 16)        # vmin = 0, vmax = 255: level k at value k
    host = si._viridis(depth, np.float32(0), np.float32(255)).astype(np.uint8)
    table = render.viridis_table()
    assert table.dtype == np.uint8 and table.shape == (256, 3)
    assert np.array_equal(host.reshape(256, 3), table)


@pytest.mark.parametrize("alpha", [0.5, 0.3, 0.77])
@pytest.mark.parametrize("n,H,W", [(0, 5, 7), (2, 3, 1), (23, 8, 12), (23, 33, 64)])
def test_restatement_is_the_host_drawing(alpha, n, H, W):
    import simple_inference as si
    frame, masks, boxes = make_case(100 * n + H, n, H, W)
    for kw in ({}, {"no_mask": True}, {"no_box": True}):
        host, _ = si.display_on_frame(_result(masks, boxes), torch.from_numpy(frame), mask_alpha=alpha, no_text=True, **kw)
        assert np.array_equal(overlay(frame, masks, boxes, alpha=alpha, **kw), host), kw
    u8 = masks.astype(np.uint8) * 255                                # byte masks: non-zero is set
    host, _ = si.display_on_frame(_result(u8, boxes), torch.from_numpy(frame), mask_alpha=alpha, no_text=True)
    assert np.array_equal(overlay(frame, u8, boxes, alpha=alpha), host)


def test_restatement_without_scores_is_the_truncated_frame():
    import simple_inference as si
    frame, masks, boxes = make_case(5, 0, 4, 6)
    r = _result(masks, boxes)
    r["pred_scores"] = None
    host, _ = si.display_on_frame(r, torch.from_numpy(frame), no_text=True)
    assert np.array_equal(overlay(frame, masks, boxes), host) and np.array_equal(host, frame.astype(np.uint8))


@pytest.mark.parametrize("name", list(HAND_MASKS))
def test_contour_rule_on_hand_made_masks(name):
    mask, outline = HAND_MASKS[name]
    assert np.array_equal(contour_of(mask), outline)
    H, W = mask.shape
    frame = np.full((H, W, 3), 10.0, np.float32)
    got = overlay(frame, mask[None], np.asarray([[0, 0, 1, 1]], np.float32), no_mask=True, no_box=True, contours=True)
    assert np.array_equal((got == 255).all(-1), outline) and np.array_equal((got == 10).all(-1), ~outline)
