#!/usr/bin/env python
"""Inference entry point (drop-in for the reference's simple_inference.py: same flags, `input:output` colon syntax,
`<name>_seg.<ext>` / `<name>_dep.png` outputs, nms / threshold overrides written into cfg.solov2).

The tensor path is the reference's: read BGR image -> resize to calc_size_preserve_ar(W, H, cfg.max_size) (cv2.INTER_LINEAR
arithmetic, no antialiasing) -> zero-pad to a multiple of 32 -> FastBaseTransform -> PlaneRecNet (eval) -> list[dict]; the
three staging steps run as one HIP launch on the uploaded uint8 frame.  The device comes from `cfg.device`.
Image file I/O and the overlay drawing use Pillow + numpy (OpenCV is not a dependency of this build).  `--render device` (not in the
reference) draws masks, boxes and the depth picture on the GPU instead (planerecnet_amd.render: the same bytes, one uint8 image each
downloaded, score texts added by Pillow afterwards); `--contours` adds white mask outlines there.  The default, `--render host`, is
unchanged.

iBims-1 exporters (`--ibims1 in:out`, `--ibims1_pd in:out`, reference simple_inference.py:202-324): every `.mat` file of `in`
(sorted; `data['rgb'][0][0]` uint8 [H,W,3], `data['calib'][0][0]` 3x3 with K = calib.T) goes through the network at its native
size (padded to a multiple of 32, outputs cropped back) and gives `out/<name>_results.mat` = {'pred_depths': float32 [H,W]} plus a
viridis preview `out/<name>_results.png`.  --ibims1 writes the predicted depth; --ibims1_pd the planar depth (planerecnet_amd.planes:
every detected plane's depth replaces the prediction under its mask), values <= 0 or >= 10 set to NaN.  Quirks kept: the `.mat`'s
rgb array enters FastBaseTransform as if it were BGR, as in the reference.  Deviation: the preview's 1 / 99 % limits come from
np.nanpercentile (the reference's np.percentile turns a NaN-holding map into a meaningless image).  scipy is needed for these
two flags only.

`--ply` (not in the reference; default off) also writes the reconstruction as a PLY triangle mesh (planerecnet_amd.reconstruct: one vertex
per pixel with a usable depth, the triangles of neighbouring pixels of one plane within --ply_gap of each other in depth): with the iBims-1
exporters `out/<name>_mesh.ply` from the depth that exporter writes, the file's RGB and the owner map of the masks; with --image
`<output>_mesh.ply`, which needs the camera as --intrinsics fx,fy,cx,cy.

`--normals` (not in the reference; default off) also writes the surface normals of the depth that run writes as a picture beside the depth
picture, `<name>_normals.png` (planerecnet_amd.normals: BGR bytes of (z, y, x) * 0.5 + 0.5, black where a pixel has no normal): tangents from
the neighbours --normals_step pixels away that lie within --normals_gap (a fraction of the smaller depth) and, where there are masks, inside
the same plane.  With --image it needs --intrinsics.  `--ply_normals` adds the same normals to --ply's file as `nx ny nz`.
"""
import argparse
import os
from pathlib import Path

import numpy as np

os.environ.setdefault("GPU_MAX_HW_QUEUES", "3")       # before the HIP runtime initialises: see planerecnet_amd/__init__.py
import torch  # noqa: E402

from planerecnet_amd.config import COLORS, cfg, set_cfg
from planerecnet_amd.funcs import calc_size_preserve_ar, frame_to_input


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="PlaneRecNet Inference (MI355X)")
    p.add_argument("--trained_model", default=None, type=str)
    p.add_argument("--config", default="PlaneRecNet_50_config")
    p.add_argument("--image", default=None, type=str, help="path or input:output")
    p.add_argument("--images", default=None, type=str, help="input_folder:output_folder")
    p.add_argument("--max_img", default=0, type=int)
    p.add_argument("--ibims1", default=None, type=str, help="in_folder:out_folder -- predicted depth of every iBims-1 .mat file -> <name>_results.mat/png")
    p.add_argument("--ibims1_pd", default=None, type=str,
                   help="in_folder:out_folder -- planar depth (each detected plane's depth under its mask, values outside (0, 10) NaN) -> <name>_results.mat/png")
    p.add_argument("--no_mask", action="store_true")
    p.add_argument("--no_box", action="store_true")
    p.add_argument("--no_text", action="store_true")
    p.add_argument("--top_k", default=100, type=int)
    p.add_argument("--nms_mode", default="matrix", type=str, choices=["matrix", "mask"])
    p.add_argument("--score_threshold", default=0.3, type=float)
    p.add_argument("--depth_mode", default="colored", type=str, choices=["colored", "gray"])
    p.add_argument("--depth_shift", default=512, type=float)
    p.add_argument("--render", default="host", type=str, choices=["host", "device"],
                   help="where masks, boxes and the depth picture are drawn: host (numpy + Pillow) or device (planerecnet_amd.render: one uint8 image each comes back)")
    p.add_argument("--contours", action="store_true", help="white one-pixel mask outlines (--render device only)")
    p.add_argument("--clean_masks", default="off", type=str, choices=["off", "largest", "all"],
                   help="reduce every predicted mask to its largest connected component, or to all components of at least --min_area pixels, "
                        "on the device (planerecnet_amd.components) before drawing and before the planar depth of --ibims1_pd")
    p.add_argument("--min_area", default=0, type=int, help="--clean_masks: components smaller than this are removed")
    p.add_argument("--fill_holes", action="store_true", help="--clean_masks: fill the holes of what was kept")
    p.add_argument("--connectivity", default=8, type=int, choices=[4, 8], help="--clean_masks: pixel connectivity of a component")
    p.add_argument("--plane_fit", default="lsq", type=str, choices=["lsq", "ransac"],
                   help="how --ibims1_pd fits each instance's plane: least squares over the whole mask, or RANSAC hypotheses scored on the device "
                        "(planerecnet_amd.planes.fit_planes_ransac) with a least-squares refit on the inliers")
    p.add_argument("--plane_threshold", default=0.05, type=float, help="--plane_fit ransac: inlier distance to the plane in metres")
    p.add_argument("--plane_relative", action="store_true", help="--plane_fit ransac: the threshold is a fraction of each pixel's depth")
    p.add_argument("--plane_hypotheses", default=256, type=int, help="--plane_fit ransac: three-point hypotheses per instance (1 .. 4096)")
    p.add_argument("--plane_refine", default=1, type=int, help="--plane_fit ransac: rounds of re-selecting the inliers and fitting again (0 .. 8)")
    p.add_argument("--plane_seed", default=0, type=int, help="--plane_fit ransac: seed of the draws")
    p.add_argument("--ply", action="store_true",
                   help="also write the reconstruction as a PLY triangle mesh (planerecnet_amd.reconstruct): out/<name>_mesh.ply with --ibims1 / --ibims1_pd, "
                        "<output>_mesh.ply with --image (which then needs --intrinsics)")
    p.add_argument("--ply_gap", default=0.05, type=float, help="--ply: the largest depth spread of a triangle's corners, as a fraction of their smallest depth")
    p.add_argument("--ply_absolute", action="store_true", help="--ply: --ply_gap is in metres")
    p.add_argument("--ply_planar_only", action="store_true", help="--ply: only pixels a detected plane owns become vertices")
    p.add_argument("--intrinsics", default=None, type=str, help="fx,fy,cx,cy of the --image file in pixels of that file (--ply)")
    p.add_argument("--normals", action="store_true",
                   help="also write the surface normals of the depth as a picture (planerecnet_amd.normals): out/<name>_normals.png with --ibims1 / --ibims1_pd, "
                        "<output>_normals.png with --image (which then needs --intrinsics)")
    p.add_argument("--normals_step", default=1, type=int, help="--normals / --ply_normals: the distance in pixels of the neighbours a tangent is taken from")
    p.add_argument("--normals_gap", default=0.05, type=float,
                   help="--normals / --ply_normals: the largest depth spread of a pixel and a neighbour it uses, as a fraction of the smaller depth")
    p.add_argument("--ply_normals", action="store_true", help="--ply: the vertices carry their pixels' normals (nx ny nz)")
    global args
    args = p.parse_args(argv)
    if args.contours and args.render != "device":
        p.error("--contours needs --render device")
    if not (args.plane_threshold > 0 and args.plane_threshold < float("inf")) or not 1 <= args.plane_hypotheses <= 4096 or not 0 <= args.plane_refine <= 8 \
            or args.plane_seed < 0:
        p.error("--plane_threshold must be positive and finite, --plane_hypotheses 1 .. 4096, --plane_refine 0 .. 8, --plane_seed >= 0")
    if args.min_area < 0:
        p.error("--min_area must be >= 0")
    if args.intrinsics is not None:
        try:
            args.intrinsics = tuple(float(v) for v in args.intrinsics.split(","))
        except ValueError:
            args.intrinsics = ()
        if len(args.intrinsics) != 4 or not all(v == v and abs(v) < float("inf") for v in args.intrinsics):
            p.error("--intrinsics must be four finite numbers fx,fy,cx,cy")
    if args.ply:
        if args.ibims1 is None and args.ibims1_pd is None and args.image is None:
            p.error("--ply goes with --ibims1, --ibims1_pd or --image")
        if args.image is not None and args.intrinsics is None:
            p.error("--ply with --image needs --intrinsics fx,fy,cx,cy: a single image carries no camera")
        if not (args.ply_gap >= 0 and args.ply_gap < float("inf")):
            p.error("--ply_gap must be finite and >= 0")
    if args.ply_normals and not args.ply:
        p.error("--ply_normals goes with --ply")
    if args.normals or args.ply_normals:
        if args.normals and args.ibims1 is None and args.ibims1_pd is None and args.image is None:
            p.error("--normals goes with --ibims1, --ibims1_pd or --image")
        if args.normals and args.image is not None and args.intrinsics is None:
            p.error("--normals with --image needs --intrinsics fx,fy,cx,cy: a single image carries no camera")
        if args.normals_step < 1 or not (args.normals_gap >= 0 and args.normals_gap < float("inf")):
            p.error("--normals_step must be >= 1, --normals_gap finite and >= 0")
    return args


def mesh_options():
    """the reconstruct.mesh keywords the --ply flags ask for"""
    return {"max_gap": args.ply_gap, "relative": not args.ply_absolute, "planar_only": args.ply_planar_only}


def normal_options():
    """the normals.from_depth keywords the --normals flags ask for"""
    return {"step": args.normals_step, "max_gap": args.normals_gap}


def ibims1_normals_path(out_folder, name):
    """<name>_normals.png in out_folder"""
    return os.path.join(out_folder, name + "_normals.png")


def write_normals(path, result, k_matrix):
    """--normals: one result dict (its "pred_plane_depth" if present, else "pred_depth"; labels = the owner map of its masks) -> the normal
    picture, made on the device: one uint8 image comes back.  -> (normals [H,W,3], valid [H,W]) on the device"""
    from planerecnet_amd import normals
    from planerecnet_amd.reconstruct import results_depth_labels
    depth, labels = results_depth_labels([result])
    n, valid, image = normals.from_depth(depth, k_matrix, labels=labels, image=True, **normal_options())
    _imwrite_bgr(path, image[0].cpu().numpy())
    return n[0], valid[0]


def ibims1_mesh_path(out_folder, name):
    """<name>_mesh.ply in out_folder"""
    return os.path.join(out_folder, name + "_mesh.ply")


def write_mesh(path, result, k_matrix, rgb, comment=None):
    """--ply: one result dict (its "pred_plane_depth" if present, else "pred_depth"; labels = the owner map of its masks) -> a PLY file;
    rgb: uint8 [H,W,3] array or tensor in the order the file shall hold"""
    from planerecnet_amd.reconstruct import reconstruct_results, write_ply
    m = reconstruct_results([result], k_matrix, frames=[torch.as_tensor(rgb)], normals=normal_options() if getattr(args, "ply_normals", False) else None,
                            **mesh_options())
    write_ply(path, m.cpu()[0], binary=True, comment=comment)


def clean_options():
    """the components.clean keywords the flags ask for (None: --clean_masks off)"""
    if args.clean_masks == "off":
        return None
    return {"keep": args.clean_masks, "min_area": args.min_area, "fill_holes": args.fill_holes, "connectivity": args.connectivity}


def robust_options():
    """the planes.fit_planes_ransac keywords the flags ask for (None: --plane_fit lsq)"""
    if args.plane_fit == "lsq":
        return None
    return {"threshold": args.plane_threshold, "relative": args.plane_relative, "hypotheses": args.plane_hypotheses, "refine": args.plane_refine,
            "seed": args.plane_seed}


def cleaned(results):
    """the network's results with the masks cleaned and the boxes recomputed where --clean_masks asks for it"""
    opts = clean_options()
    if opts is None:
        return results
    from planerecnet_amd.components import clean_results
    return clean_results(results, **opts)


def _imread_bgr(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1].copy()


def _imwrite_bgr(path, arr):
    from PIL import Image
    if arr.ndim == 3:
        Image.fromarray(arr[:, :, ::-1].astype(np.uint8)).save(path)
    elif arr.dtype == np.uint16:
        Image.fromarray(arr.astype(np.uint16)).save(path)
    else:
        Image.fromarray(arr.astype(np.uint8)).save(path)


def display_on_frame(result, frame, mask_alpha=0.5, no_mask=False, no_box=False, no_text=False):
    """Blend instance masks / boxes / scores over the (padded) BGR frame; returns (uint8 HxWx3 BGR, depth HxW float)."""
    from PIL import Image, ImageDraw
    depth = result["pred_depth"].squeeze().float().cpu().numpy()
    img = frame.float().cpu().numpy()
    if result["pred_scores"] is None:
        return img.astype(np.uint8), depth
    masks = result["pred_masks"].cpu().numpy()
    for i in range(masks.shape[0] - 1, -1, -1):
        if not no_mask:
            color = np.asarray(COLORS[(i * 5) % len(COLORS)][::-1], np.float32)      # stored RGB, frame is BGR
            m = masks[i][..., None]
            img = np.where(m, img * (1 - mask_alpha) + color * mask_alpha, img)
    pil = Image.fromarray(img[:, :, ::-1].astype(np.uint8))
    draw = ImageDraw.Draw(pil)
    boxes, scores = result["pred_boxes"].cpu().numpy(), result["pred_scores"].cpu().numpy()
    for i in range(masks.shape[0]):
        x0, y0, x1, y1 = [int(v) for v in boxes[i]]
        if not no_box:
            draw.rectangle([x0, y0, x1, y1], outline=COLORS[(i * 5) % len(COLORS)], width=1)
        if not no_text:
            draw.text((x0 + 2, y0 + 2), "plane: %.2f" % scores[i], fill=(255, 255, 255))
    return np.asarray(pil)[:, :, ::-1], depth


def display_on_device(result, frame, depth_mode="colored", depth_shift=512, no_mask=False, no_box=False, no_text=False, contours=False):
    """display_on_frame and the depth picture with the drawing on the device (planerecnet_amd.render): masks, outlines, boxes and the
    depth colours are made there, ONE uint8 image and ONE depth image are downloaded; the score texts are then drawn on the downloaded
    image by Pillow -- all of them after all boxes (display_on_frame draws text i before box i + 1, so a later box can cross an earlier
    text there).  -> (uint8 HxWx3 BGR, depth image: uint8 HxWx3 BGR or uint16 HxW)"""
    from planerecnet_amd import render
    seg = render.render_overlay(result, frame, no_mask=no_mask, no_box=no_box, contours=contours)
    dep = render.colorize_depth(result["pred_depth"], mode=depth_mode, depth_shift=depth_shift)
    seg, dep = seg.cpu().numpy(), dep.cpu().numpy()
    if not no_text and result["pred_scores"] is not None:
        from PIL import Image, ImageDraw
        pil = Image.fromarray(seg[:, :, ::-1])
        draw = ImageDraw.Draw(pil)
        boxes, scores = result["pred_boxes"].cpu().numpy(), result["pred_scores"].cpu().numpy()
        for i in range(scores.shape[0]):
            draw.text((int(boxes[i][0]) + 2, int(boxes[i][1]) + 2), "plane: %.2f" % scores[i], fill=(255, 255, 255))
        seg = np.asarray(pil)[:, :, ::-1]
    return seg, dep


def _viridis(depth, vmin, vmax):
    """depth clipped to [vmin, vmax], stretched to 0..255 and mapped through a 5-stop viridis ramp -> uint8 [H,W,3] RGB"""
    d = depth.clip(min=vmin, max=vmax)
    lo, hi = (np.nanmin(d), np.nanmax(d)) if np.isfinite(d).any() else (0.0, 0.0)
    d = np.nan_to_num((d - lo) / max(hi - lo, 1e-12) * 255, nan=0.0).astype(np.uint8)
    return np.stack([np.interp(d, [0, 64, 128, 192, 255], c) for c in ([68, 59, 33, 94, 253], [1, 82, 145, 201, 231], [84, 139, 140, 98, 37])], -1)


@torch.no_grad()
def inference_image(net, path, save_path=None, depth_mode="colored"):
    frame_np = _imread_bgr(path)
    H, W, _ = frame_np.shape
    # the decoded frame goes to the device as BYTES (page-locked, asynchronous); resize (cv2.INTER_LINEAR arithmetic), zero
    # padding to a multiple of 32 and FastBaseTransform are one HIP launch there (planerecnet_amd.funcs.frame_to_input)
    staged = torch.from_numpy(np.ascontiguousarray(frame_np))
    if torch.cuda.is_available():
        staged = staged.pin_memory()
    batch, frame = frame_to_input(staged.to(cfg.device, non_blocking=True), calc_size_preserve_ar(W, H, cfg.max_size))
    results = cleaned(net(batch))
    name, ext = os.path.splitext(path if save_path is None else save_path)
    save_path = name + "_seg" + ext if save_path is None else save_path
    depth_path = name + "_dep.png"
    if args.ply or getattr(args, "normals", False):
        # the depth lives on the resized (and zero-padded) frame: the mesh is cut to the resized picture, the intrinsics follow the resize
        # (pixel centres: x' = (x + 0.5) s - 0.5), the colours are that picture's
        Wr, Hr = calc_size_preserve_ar(W, H, cfg.max_size)
        fx, fy, cx, cy = args.intrinsics
        sx, sy = Wr / W, Hr / H
        k_matrix = np.array([[fx * sx, 0.0, (cx + 0.5) * sx - 0.5], [0.0, fy * sy, (cy + 0.5) * sy - 0.5], [0.0, 0.0, 1.0]])
        r = dict(results[0])
        r["pred_depth"] = r["pred_depth"][..., :Hr, :Wr]
        if r.get("pred_masks") is not None:
            r["pred_masks"] = r["pred_masks"][:, :Hr, :Wr]
        if args.ply:
            rgb = frame[:Hr, :Wr].flip(-1).round().clamp(0, 255).to(torch.uint8)
            write_mesh(os.path.splitext(save_path)[0] + "_mesh.ply", r, k_matrix, rgb, comment="PlaneRecNet " + os.path.basename(path))
        if getattr(args, "normals", False):
            write_normals(name + "_normals.png", r, k_matrix)
    if args.render == "device":
        blended, depth_image = display_on_device(results[0], frame, depth_mode=depth_mode, depth_shift=args.depth_shift, no_mask=args.no_mask,
                                                 no_box=args.no_box, no_text=args.no_text, contours=args.contours)
        _imwrite_bgr(save_path, blended)
        _imwrite_bgr(depth_path, depth_image)
        return results
    blended, depth = display_on_frame(results[0], frame, no_mask=args.no_mask, no_box=args.no_box, no_text=args.no_text)
    _imwrite_bgr(save_path, blended)
    if depth_mode == "colored":
        vmin, vmax = np.percentile(depth, 1), np.percentile(depth, 99)
        _imwrite_bgr(depth_path, _viridis(depth, vmin, vmax)[:, :, ::-1])
    else:
        _imwrite_bgr(depth_path, (depth * args.depth_shift).astype(np.uint16))
    return results


def inference_images(net, in_folder, out_folder, max_img=0, depth_mode="colored"):
    os.makedirs(out_folder, exist_ok=True)
    files = sorted(p for p in Path(in_folder).glob("*") if p.suffix in (".png", ".jpg"))
    for i, p in enumerate(files[: max_img if max_img > 0 else len(files)]):
        inference_image(net, str(p), os.path.join(out_folder, p.name), depth_mode=depth_mode)
        print("Inference images: " + p.name, end="\r")
    print("\nDone.")


def _scipy_io():
    try:
        import scipy.io
    except ImportError:
        raise SystemExit("--ibims1 / --ibims1_pd read and write MATLAB files and need scipy (scipy.io), which is not installed.")
    return scipy.io


def read_ibims1_mat(path):
    """an iBims-1 .mat file -> (rgb uint8 [H,W,3], K float64 [3,3]); the file stores the intrinsics transposed (K = calib.T)"""
    data = _scipy_io().loadmat(path)["data"]
    rgb = np.ascontiguousarray(data["rgb"][0][0], dtype=np.uint8)
    return rgb, np.asarray(data["calib"][0][0], dtype=np.float64).T.copy()


def ibims1_inputs(in_folder):
    """the .mat files of in_folder, sorted, as (name, path)"""
    return [(p.stem, str(p)) for p in sorted(Path(in_folder).glob("*")) if p.suffix == ".mat"]


def ibims1_outputs(out_folder, name):
    """(<name>_results.mat, <name>_results.png) in out_folder"""
    base = os.path.join(out_folder, name + "_results")
    return base + ".mat", base + ".png"


@torch.no_grad()
def ibims1_results(net, rgb):
    """one iBims-1 frame through the network at native size: the rgb array enters as if it were BGR (the reference's quirk), the
    input is zero-padded to a multiple of 32 and the outputs are cropped back -> the eval-mode result dict of the frame"""
    H, W, _ = rgb.shape
    staged = torch.from_numpy(rgb)
    if torch.cuda.is_available():
        staged = staged.pin_memory()
    batch, _ = frame_to_input(staged.to(cfg.device, non_blocking=True), (W, H), want_frame=False)
    r = dict(net(batch)[0])
    r["pred_depth"] = r["pred_depth"][..., :H, :W]
    if r["pred_masks"] is not None:
        r["pred_masks"] = r["pred_masks"][:, :H, :W]
    return r


def _ibims1_export(net, in_folder, out_folder, planar):
    sio = _scipy_io()
    os.makedirs(out_folder, exist_ok=True)
    for name, path in ibims1_inputs(in_folder):
        rgb, k_matrix = read_ibims1_mat(path)
        r = ibims1_results(net, rgb)
        if planar:
            from planerecnet_amd.planes import planar_depth
            planar_out = planar_depth([r], k_matrix, depth_range=(0.0, 10.0), clean=clean_options(), robust=robust_options())[0]
            depth = planar_out["pred_plane_depth"]
        else:
            depth = r["pred_depth"]
        if args.ply or getattr(args, "normals", False):
            shown = dict(r)
            if planar:
                shown.update({k: v for k, v in planar_out.items() if k in ("pred_plane_depth", "pred_plane_masks")})
        if getattr(args, "normals", False):
            write_normals(ibims1_normals_path(out_folder, name), shown, k_matrix)
        if args.ply:
            write_mesh(ibims1_mesh_path(out_folder, name), shown, k_matrix, rgb, comment="PlaneRecNet " + os.path.basename(path))
        depth = depth.squeeze().float().cpu().numpy()
        out, preview = ibims1_outputs(out_folder, name)
        sio.savemat(out, {"pred_depths": depth})
        if np.isfinite(depth).any():
            vmin, vmax = np.nanpercentile(depth, 1), np.nanpercentile(depth, 99)
        else:
            vmin = vmax = 0.0
        _imwrite_bgr(preview, _viridis(depth, vmin, vmax)[:, :, ::-1])
        print(os.path.basename(path) + " -> " + os.path.basename(out), end="\r")
    print("\nDone.")


def ibims1(net, in_folder, out_folder):
    """--ibims1: the predicted depth of every iBims-1 .mat file (reference simple_inference.py:202-236)"""
    _ibims1_export(net, in_folder, out_folder, planar=False)


def ibims1_pd(net, in_folder, out_folder):
    """--ibims1_pd: the planar depth, values <= 0 or >= 10 NaN (reference simple_inference.py:240-324)"""
    _ibims1_export(net, in_folder, out_folder, planar=True)


def main(argv=None):
    parse_args(argv)
    torch.set_num_threads(4)                                   # host-side tensor ops are small: a wide OpenMP team only adds fork / join latency (as train.py)
    from planerecnet_amd import timer
    from planerecnet_amd.planerecnet import PlaneRecNet
    timer.disable_all()
    set_cfg(args.config)
    # the reference feeds --score_threshold into BOTH mask_thr and update_thr (quirk Q12)
    cfg.solov2.replace({"nms_type": args.nms_mode, "mask_thr": args.score_threshold, "update_thr": args.score_threshold, "top_k": args.top_k})
    if not torch.cuda.is_available():
        raise SystemExit("No GPU detected: the HIP path has no CPU fallback.")
    cfg.device = "cuda:0" if cfg.device == "cuda" else cfg.device
    net = PlaneRecNet(cfg)
    if args.trained_model is not None:
        net.load_weights(args.trained_model)
    else:
        backbone = "weights/" + cfg.backbone.path
        if os.path.exists(backbone):
            net.init_weights(backbone_path=backbone)
        else:
            net.init_head_weights()
        print(cfg.backbone.name)
    net.train(mode=False)
    net = net.to(cfg.device)
    if args.ibims1 is not None:
        inp, out = args.ibims1.split(":")
        ibims1(net, inp, out)
    if args.ibims1_pd is not None:
        inp, out = args.ibims1_pd.split(":")
        ibims1_pd(net, inp, out)
    if args.image is not None:
        inp, out = args.image.split(":") if ":" in args.image else (args.image, None)
        print("Inference image: {}".format(inp))
        inference_image(net, inp, out, depth_mode=args.depth_mode)
    if args.images is not None:
        inp, out = args.images.split(":")
        inference_images(net, inp, out, max_img=args.max_img, depth_mode=args.depth_mode)


if __name__ == "__main__":
    main()
