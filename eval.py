#!/usr/bin/env python
"""Evaluation entry point (reference eval.py): the same flags, the same loop -- one frame at a time through the eval-mode
network, depth errors and box / mask AP at IoU .50 ... .95 accumulated over the frames, mAP table and mean depth errors
printed at the end -- and `evaluate(net, dataset, during_training, eval_nums)` for train.py's validation pass.

What differs underneath: the network and its post-process run on the HIP kernels; per frame, the depth errors are one fused
reduction and the two pairwise IoU matrices one popcount kernel (planerecnet_amd/metrics.py; include/prn.h:
prn_depth_metrics, prn_pairwise_iou); only the per-threshold matching and the AP integral -- a few hundred scalar
operations -- run on the host.

Outside this build (they need cv2 / pycocotools / tensorboardX): the annotated dataset readers -- frames come from
`--dataset synthetic` (planerecnet_amd/datasets.py) -- and `--autopsy`.

`--output_coco_json` writes every detection of every evaluated frame as COCO result files (YOLACT's `Detections`; the reference parses
the flag and drops it): boxes to `--bbox_det_file`, masks to `--mask_det_file` as compressed run-length strings coded on the device
(planerecnet_amd/rle.py; include/prn.h: prn_rle_*) -- the masks themselves never leave the GPU.  Without the flag nothing is collected.

`--boundary_ap` adds a third row, `bndry`, to the AP table: Boundary AP in COCO's form (Cheng et al., CVPR 2021), where a detection matches a
ground-truth mask iff min(mask IoU, boundary IoU) exceeds the threshold.  The bands (`--boundary_ratio` of the image diagonal wide) are eroded
and compared on the device (planerecnet_amd/morphology.py, metrics.boundary_iou; include/prn.h: prn_boundary_iou).  Without the flag the
output is what it was.

`--plane_metrics` adds the plane-level figures of the PlaneNet / PlaneRCNN / PlaneRecNet tables: the segmentation scores RI, VOI and SC, and
plane and pixel recall at depth-error thresholds 0.05 .. 1.0 m.  Per frame the masks are painted into two label maps and reduced to one small
integer table on the device (planerecnet_amd/plane_eval.py; include/prn.h: prn_label_map, prn_label_overlap); the tables come down once, after
the last frame.  Without the flag the output and the return value are what they were.

`--normal_metrics` adds the surface-normal figures such work is judged by: the mean, median and RMS angle between the normals of the predicted
depth and of the ground-truth depth -- the pair the depth errors compare, under the dataset's intrinsics, no labels -- and the shares of pixels
within 11.25 / 22.5 / 30 degrees, pooled over all frames' pixels.  Both normal maps and the error histogram are computed on the device
(planerecnet_amd/normals.py; include/prn.h: prn_normals, prn_normal_error); the tables come down once, after the last frame.  No median scaling:
under the relative gap (`--normal_gap`, a fraction of the smaller depth) the normals do not depend on a global depth scale.  Without the flag the
output and the return value are what they were.
"""
import argparse
import json
import os
import random
import time

import numpy as np

os.environ.setdefault("GPU_MAX_HW_QUEUES", "3")       # before the HIP runtime initialises: see planerecnet_amd/__init__.py
import torch  # noqa: E402

from planerecnet_amd.config import cfg, set_cfg, set_dataset  # noqa: E402
from planerecnet_amd.utils import MovingAverage, SavePath  # noqa: E402

args = None


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="PlaneRecNet Evaluation (MI355X)")
    parser.add_argument("--trained_model", default=None, type=str,
                        help='Trained state_dict file path to open ("interrupt" / "latest" / path; none: random initialisation).')
    parser.add_argument("--top_k", default=100, type=int, help="Further restrict the number of predictions to parse")
    parser.add_argument("--score_threshold", default=0.15, type=float, help="Detections with a score under this threshold will not be considered.")
    parser.add_argument("--nms_mode", default="matrix", type=str, choices=["matrix", "mask"], help="Chose NMS type from matrix and mask nms.")
    parser.add_argument("--output_coco_json", dest="output_coco_json", action="store_true",
                        help="Write the detections of the evaluated frames as COCO result files (see --bbox_det_file / --mask_det_file).")
    parser.add_argument("--bbox_det_file", default="results/bbox_detections.json", type=str,
                        help="With --output_coco_json: the file the box detections go to (image_id, category_id, bbox [x, y, w, h], score).")
    parser.add_argument("--mask_det_file", default="results/mask_detections.json", type=str,
                        help="With --output_coco_json: the file the mask detections go to (image_id, category_id, segmentation as COCO RLE, score).")
    parser.add_argument("--max_images", default=-1, type=int, help="The maximum number of images from the dataset to consider. Use -1 for all.")
    parser.add_argument("--config", default=None, help="The config object to use.")
    parser.add_argument("--no_bar", dest="no_bar", action="store_true", help="Do not output the status bar.")
    parser.add_argument("--autopsy", dest="autopsy", action="store_true", help="(tensorboard image log: not part of this build)")
    parser.add_argument("--dataset", default=None, type=str, help="Override the config's dataset ('synthetic' for seeded synthetic frames).")
    parser.add_argument("--boundary_ap", dest="boundary_ap", action="store_true",
                        help="(extension) Add a Boundary AP row to the table: a detection matches iff min(mask IoU, boundary IoU) exceeds the threshold.")
    parser.add_argument("--boundary_ratio", default=0.02, type=float,
                        help="With --boundary_ap: the band width as a share of the image diagonal (Boundary IoU's dilation ratio).")
    parser.add_argument("--plane_metrics", dest="plane_metrics", action="store_true",
                        help="(extension) Add the plane segmentation scores RI / VOI / SC and plane / pixel recall over depth-error thresholds.")
    parser.add_argument("--normal_metrics", dest="normal_metrics", action="store_true",
                        help="(extension) Add the angular error of the predicted depth's surface normals against the ground-truth depth's.")
    parser.add_argument("--normal_step", default=1, type=int, help="With --normal_metrics: the neighbours' distance in pixels.")
    parser.add_argument("--normal_gap", default=0.05, type=float,
                        help="With --normal_metrics: the largest depth spread of a pixel and a neighbour it uses, as a fraction of the smaller depth.")
    parser.add_argument("--synthetic_size", default=16, type=int, help="(extension) frames in the synthetic dataset.")
    global args
    args = parser.parse_args(argv)
    return args


def _bar(done, total, width=30):
    filled = int(round(width * done / max(total, 1)))
    return "[" + "#" * filled + " " * (width - filled) + "]"


class Detections:
    """The detections of the evaluated frames in COCO's result format (YOLACT eval.py: `Detections`): two lists, written as two JSON files.
      bbox_data  {"image_id", "category_id", "bbox": [x, y, w, h], "score"}: pred_boxes (x0, y0, x1, y1) as [x0, y0, x1 - x0, y1 - y0], every
                 value rounded to one decimal
      mask_data  {"image_id", "category_id", "segmentation": {"size": [H, W], "counts": str}, "score"}: the mask as compressed RLE
    `encode`: masks [N,H,W] -> N RLE dicts (default: planerecnet_amd.rle.encode, on the device)."""

    def __init__(self, encode=None):
        self.bbox_data, self.mask_data = [], []
        self._encode = encode

    def add_frame(self, image_id, result, label_map=None):
        """every detection of one eval-mode result dict; a frame without detections adds nothing"""
        masks = result.get("pred_masks")
        if masks is None or result.get("pred_scores") is None or len(masks) == 0:
            return
        if self._encode is None:
            from planerecnet_amd import rle
            self._encode = rle.encode
        rles = self._encode(masks)
        boxes, classes, scores = (torch.as_tensor(result[k]).cpu().tolist() for k in ("pred_boxes", "pred_classes", "pred_scores"))
        label_map = label_map or {}
        image_id = image_id.item() if hasattr(image_id, "item") else image_id        # (a numpy / tensor scalar id: json takes plain ints)
        for box, cls, score, seg in zip(boxes, classes, scores, rles):
            category = label_map.get(int(cls) + 1, int(cls) + 1)
            bbox = [box[0], box[1], box[2] - box[0], box[3] - box[1]]
            self.bbox_data.append({"image_id": image_id, "category_id": category, "bbox": [round(float(v) * 10) / 10 for v in bbox], "score": float(score)})
            self.mask_data.append({"image_id": image_id, "category_id": category, "segmentation": {"size": list(seg["size"]), "counts": seg["counts"]},
                                   "score": float(score)})

    def dump(self, bbox_file, mask_file):
        for data, path in ((self.bbox_data, bbox_file), (self.mask_data, mask_file)):
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                json.dump(data, f)


def evaluate(net, dataset, during_training=False, eval_nums=-1, detections=None, boundary_ratio=None, plane_metrics=False, normal_metrics=False):
    """Reference eval.py:63-130.  Returns (mAP table as calc_map returns it, {metric name: mean over the frames}).
    detections: a `Detections` collector every frame's detections are added to (eval.py --output_coco_json; train.py passes none).
    boundary_ratio: add the Boundary AP row (eval.py --boundary_ap); the band width of a frame is this share of its ground-truth masks' diagonal.
    plane_metrics: add RI / VOI / SC and the plane / pixel recall curves (eval.py --plane_metrics) to the printout and, under the keys `RI`, `VOI`,
    `SC`, `plane_recall`, `pixel_recall`, to the returned metrics.
    normal_metrics: add the angular error of the predicted depth's normals against the ground-truth depth's (eval.py --normal_metrics; step and gap
    from --normal_step / --normal_gap) to the printout and, under the keys `normal_mean`, `normal_median`, `normal_rmse`, `normal_11.25`, `normal_22.5`,
    `normal_30`, `normal_pixels`, to the returned metrics."""
    from planerecnet_amd import metrics
    from planerecnet_amd.morphology import boundary_radius
    if args is None:
        parse_args(["--no_bar"])                                    # train.py's setup_eval (reference train.py:436-437)
    frame_times = MovingAverage()
    eval_nums = len(dataset) - 1 if eval_nums < 0 else min(eval_nums, len(dataset))     # (the reference's "- 1" included)
    print()
    indices = list(range(len(dataset)))
    random.shuffle(indices)
    indices = indices[:eval_nums]
    dev = next(net.parameters()).device
    infos, ap_data, all_maps = [], metrics.new_ap_data(boundary=boundary_ratio is not None), None
    planes = None
    if plane_metrics:
        from planerecnet_amd.plane_eval import PlaneEvalAccumulator
        planes = PlaneEvalAccumulator()
    normal_acc = None
    if normal_metrics:
        from planerecnet_amd import normals
        normal_acc = normals.NormalErrorAccumulator((11.25, 22.5, 30), device=dev)
        normal_kw = {"step": getattr(args, "normal_step", 1), "max_gap": getattr(args, "normal_gap", 0.05)}
    try:
        for it, image_idx in enumerate(indices):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            image, gt_instances, gt_depth = dataset.pull_item(image_idx)
            result = net(image.unsqueeze(0).to(dev))[0]
            gt_masks, gt_boxes, gt_classes = (gt_instances[k].to(dev) for k in ("masks", "boxes", "classes"))
            infos.append([float(v) for v in metrics.compute_depth_metrics(result["pred_depth"], gt_depth.to(dev), median_scaling=True)])
            if planes is not None:                                  # (a frame without detections counts: nothing is recalled in it)
                planes.add_frame(gt_masks, gt_depth.to(dev), result["pred_masks"], result["pred_depth"])
            if normal_acc is not None:
                maps = [normals.from_depth(d.float().reshape(d.shape[-2:]), gt_instances["k_matrix"], **normal_kw) for d in (result["pred_depth"], gt_depth.to(dev))]
                normal_acc.add(maps[0][0], maps[0][1], maps[1][0], maps[1][1])
            if result["pred_masks"] is not None:
                radius = None if boundary_ratio is None else boundary_radius(gt_masks.shape[-2], gt_masks.shape[-1], boundary_ratio)
                metrics.compute_segmentation_metrics(ap_data, gt_masks, gt_boxes, gt_classes, result["pred_masks"], result["pred_boxes"],
                                                     result["pred_classes"], result["pred_scores"], boundary_radius=radius)
                if detections is not None:
                    image_id = dataset.ids[image_idx] if hasattr(dataset, "ids") else image_idx
                    detections.add_frame(image_id, result, getattr(cfg.dataset, "label_map", None))
            torch.cuda.synchronize(dev)
            if it > 1:                                              # the first frames include one-time setup (reference :103-106)
                frame_times.add(time.perf_counter() - t0)
            if not args.no_bar:
                fps = 1.0 / frame_times.get_avg() if it > 1 else 0
                print("\rProcessing Images  %s %6d / %6d (%5.2f%%)    %5.2f fps        "
                      % (_bar(it + 1, eval_nums), it + 1, eval_nums, (it + 1) / eval_nums * 100, fps), end="")
        all_maps = metrics.calc_map(ap_data)
        mean = np.asarray(infos, dtype=np.double).sum(axis=0) / max(len(infos), 1) if infos else np.zeros(8)
        print()
        print("Depth Metrics:")
        names = metrics.depth_metrics
        print(", ".join("{}: {:.5f}".format(n, v) for n, v in zip(names[:7], mean[:7])) + " \n{}: {:.5f}".format(names[7], mean[7]))
        depth_metrics = dict(zip(names, mean.tolist()))
        if planes is not None:
            res = planes.result()
            print("Plane segmentation: RI: {:.5f}, VOI: {:.5f}, SC: {:.5f}".format(res["RI"], res["VOI"], res["SC"]))
            print("depth m | " + " ".join("{:5.2f}".format(t) for t in res["thresholds"][1:]))
            for row, key in (("plane", "plane_recall"), ("pixel", "pixel_recall")):
                print("{:>7} | ".format(row) + " ".join("{:5.3f}".format(v) for v in res[key][1:]))
            depth_metrics.update({k: res[k] for k in ("RI", "VOI", "SC", "plane_recall", "pixel_recall")})
        if normal_acc is not None:
            res = normal_acc.result()
            print("Normal Metrics:")
            print("mean: {:.5f}, median: {:.5f}, rmse: {:.5f}, 11.25: {:.5f}, 22.5: {:.5f}, 30: {:.5f}".format(res["mean"], res["median"], res["rmse"], *res["within"]))
            depth_metrics.update({"normal_mean": res["mean"], "normal_median": res["median"], "normal_rmse": res["rmse"], "normal_11.25": float(res["within"][0]),
                                  "normal_22.5": float(res["within"][1]), "normal_30": float(res["within"][2]), "normal_pixels": res["count"]})
        return all_maps, depth_metrics
    except KeyboardInterrupt:
        print("Stopping...")
        return all_maps, {}


def main():
    parse_args()
    torch.set_num_threads(4)                                   # host-side tensor ops are small: a wide OpenMP team only adds fork / join latency (as train.py)
    if args.autopsy:
        raise SystemExit("eval.py: --autopsy writes tensorboard images (tensorboardX + cv2 colour maps); not part of this build")
    if args.trained_model == "interrupt":
        args.trained_model = SavePath.get_interrupt("weights/")
    elif args.trained_model == "latest":
        if args.config is None:
            raise SystemExit("eval.py: --trained_model latest needs --config")
        set_cfg(args.config)
        args.trained_model = SavePath.get_latest("weights/", cfg.name)
    if args.config is None:
        if args.trained_model is None:
            raise SystemExit("eval.py: give --config (or a --trained_model whose file name carries it)")
        args.config = SavePath.from_str(args.trained_model).model_name + "_config"
        print("Config not specified. Parsed %s from the file name.\n" % args.config)
    set_cfg(args.config)
    cfg.solov2.replace({"nms_type": args.nms_mode, "mask_thr": args.score_threshold, "update_thr": args.score_threshold, "top_k": args.top_k})
    if args.dataset not in (None, "synthetic"):
        set_dataset(args.dataset)
    if not torch.cuda.is_available():
        raise SystemExit("No GPUs detected. The HIP path has no CPU fallback.")
    from planerecnet_amd import timer
    from planerecnet_amd.datasets import SyntheticPlaneDataset
    from planerecnet_amd.planerecnet import PlaneRecNet
    if args.dataset != "synthetic":
        # never print metrics of seeded noise frames under a real dataset's name: the reference fails on a missing dataset too
        raise SystemExit("eval.py: the annotated dataset readers (cv2 + pycocotools) are outside this build; pass --dataset synthetic "
                         "to evaluate on seeded synthetic frames (the numbers then say nothing about a trained model's accuracy).")
    print("NOTE: evaluating on SYNTHETIC frames (--dataset synthetic): the metrics below are plumbing checks, not accuracy figures.")
    dataset = SyntheticPlaneDataset(args.synthetic_size)
    with torch.no_grad():
        os.makedirs("results", exist_ok=True)
        print("Loading model...", end="")
        torch.manual_seed(0)
        net = PlaneRecNet(cfg)
        if args.trained_model is not None:
            net.load_weights(args.trained_model)
        else:
            net.init_head_weights()
            print(" (no --trained_model: random initialisation)", end="")
        net.eval()
        timer.disable_all()
        print(" done.")
        cfg.device = "cuda:0"
        net = net.to("cuda:0")
        detections = Detections() if args.output_coco_json else None
        evaluate(net, dataset, during_training=False, eval_nums=args.max_images, detections=detections,
                 boundary_ratio=args.boundary_ratio if args.boundary_ap else None, plane_metrics=args.plane_metrics, normal_metrics=args.normal_metrics)
        if detections is not None:
            detections.dump(args.bbox_det_file, args.mask_det_file)
            print("Wrote %d detections to %s and %s" % (len(detections.bbox_data), args.bbox_det_file, args.mask_det_file))


if __name__ == "__main__":
    main()
