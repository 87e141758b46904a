"""Golden vectors for the planar depth of the iBims-1 exporter -- runs ONLY in the build container (needs the reference).

    python tests/golden/make_golden_planes.py

Writes two seeded synthetic iBims-1 style `.mat` files (rgb + calib), runs the reference's own `simple_inference.ibims1_pd`
(simple_inference.py:240-324) on them with a stub network that returns fixed `pred_depth` / `pred_masks` (near-planar depth with
noise, overlapping masks, one instance whose plane leaves (0, 10) so that the NaN rule applies), checks that the fp64
restatement (tests/planes_restate.py) reproduces the reference's `pred_depths`, and stores inputs and outputs in
tests/golden/plane_depth.npz.  Local stubs on top of oracle.ref_shim: numpy.core.numeric.NaN (removed in numpy 2) and no-op
cv2.applyColorMap / cv2.imwrite (the preview image is not part of the fixture)."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_shim  # noqa: E402
from planes_restate import k_of, plane_depth_map, restate  # noqa: E402

H, W = 120, 160


def make_image(seed):
    """(rgb, calib, depth [H,W] fp32, masks [N,H,W] bool)"""
    rng = np.random.RandomState(500 + seed)
    K = k_of(140.0 + 10 * seed, 135.0 + 5 * seed, 79.5 + 2 * seed, 59.5 - seed)
    depth = plane_depth_map([0.0, 0.0, 1.0], 4.0 + seed, K, H, W)                       # fronto-parallel background
    masks = []

    def add_plane(n, d, y0, y1, x0, x1, ellipse=False):
        n = np.asarray(n, np.float64) / np.linalg.norm(n)
        pd = plane_depth_map(n, d, K, H, W)
        m = np.zeros((H, W), bool)
        if ellipse:
            yy, xx = np.mgrid[:H, :W]
            m = ((yy - (y0 + y1) / 2) / ((y1 - y0) / 2)) ** 2 + ((xx - (x0 + x1) / 2) / ((x1 - x0) / 2)) ** 2 <= 1
        else:
            m[y0:y1, x0:x1] = True
        m &= np.abs(pd) < 40                                                            # (finite input depth: the horizon of a plane stays out)
        depth[m] = pd[m]
        masks.append(m)
    add_plane([0.0, 1.0, 0.05], 1.5, 80, 120, 0, 160)                                  # floor: 10 m at its far edge
    add_plane([-1.0, 0.05, 0.1], 2.0 + 0.3 * seed, 10, 90, 0, 45)                       # left wall
    add_plane([-0.2, 0.1, 1.0], 3.0, 30, 70, 50, 110, ellipse=True)                     # a board, overlapping ...
    add_plane([0.1, -0.2, 1.0], 2.5, 50, 95, 90, 140)                                   # ... this box and the floor
    add_plane([1.0, 0.0, -0.25], 0.1, 5, 60, 100, 160)                                  # nearly along the rays: leaves (0, 10) on both sides
    depth = depth * (1.0 + 0.01 * rng.randn(H, W))                                      # 1 % noise: near-planar
    masks = np.stack(masks)
    for i in range(len(masks)):                                                         # ragged edges
        masks[i] &= rng.rand(H, W) > 0.03
    if seed == 1:
        masks = masks[[0, 2, 3, 4, 1]]                                                  # another composition order
    rgb = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    return rgb, K.T.copy(), depth.astype(np.float32), masks


def main():
    ref_shim.install()
    import numpy.core.numeric as ncn
    ncn.NaN = np.nan
    import cv2
    cv2.COLORMAP_VIRIDIS = 16
    cv2.applyColorMap = lambda img, cmap: img
    cv2.imwrite = lambda path, img: True
    ref_shim.load_reference()
    import scipy.io
    import simple_inference as rsi

    images = [make_image(s) for s in (0, 1)]
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        in_dir, out_dir = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        os.makedirs(in_dir)
        for s, (rgb, calib, _, _) in enumerate(images):
            scipy.io.savemat(os.path.join(in_dir, "img%d.mat" % s), {"data": {"rgb": rgb, "calib": calib}})
        it = iter(images)

        def stub_net(batch):
            _, _, depth, masks = next(it)
            assert tuple(batch.shape) == (1, 3, H, W)
            return [{"pred_depth": torch.from_numpy(depth)[None, None], "pred_masks": torch.from_numpy(masks)}]
        rsi.ibims1_pd(stub_net, in_dir, out_dir)
        for s in range(len(images)):
            outs.append(scipy.io.loadmat(os.path.join(out_dir, "img%d_results.mat" % s))["pred_depths"])
    for (rgb, calib, depth, masks), ref in zip(images, outs):
        assert ref.dtype == np.float32 and ref.shape == (H, W)
        mine, _, valid = restate(depth, masks, calib.T, depth_range=(0.0, 10.0))
        assert bool(valid.all())
        assert np.array_equal(np.isnan(mine), np.isnan(ref)), "NaN pattern"
        f = ~np.isnan(ref)
        err = float(np.max(np.abs(mine[f].astype(np.float64) - ref[f]) / np.abs(ref[f])))
        assert err <= 1e-12, err
        print("restatement vs reference: max rel err %.3g, NaN pixels %d, masks %d" % (err, int((~f).sum()), len(masks)))
    data = {"calib": np.stack([im[1] for im in images]), "depth": np.stack([im[2] for im in images]), "pred_depths": np.stack(outs)}
    for s, im in enumerate(images):
        data["masks%d" % s] = im[3]
    np.savez_compressed(os.path.join(HERE, "plane_depth.npz"), **data)
    print("wrote", os.path.join(HERE, "plane_depth.npz"))


if __name__ == "__main__":
    main()
