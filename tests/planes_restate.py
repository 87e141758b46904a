"""fp64 restatement of the plane fit and planar depth of the reference's iBims-1 exporter (simple_inference.py:240-324,
PCA_svd of models/functions/funcs.py:287-291), with the same torch operations in the same order on the CPU, plus this
build's rule for instances the reference cannot fit (fewer than 3 pixels, degenerate scatter: invalid, no part in the
composition).  Used by tests/test_planes_cpu.py (against the golden fixture) and tests/test_planes_gpu.py (against the device)."""
import numpy as np
import torch


def restate(depth, masks, k_matrix, depth_range=None):
    """depth [H,W] fp32, masks [N,H,W] bool, k_matrix [3,3] (= calib.T) ->
    (plane depth [H,W] fp32 numpy, planes [N,4] fp64 (nx, ny, nz, d) with d >= 0 and NaN rows for invalid instances, valid [N] bool)"""
    depth = torch.as_tensor(depth, dtype=torch.float32)
    masks = torch.as_tensor(masks).bool()
    H, W = depth.shape
    k = torch.as_tensor(k_matrix, dtype=torch.float64)
    intrinsic_inv = torch.inverse(k)
    cx, cy, fx, fy = k[0][2], k[1][2], k[0][0], k[1][1]
    v, u = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    Z = depth.unsqueeze(0)
    X = (u - cx) * Z / fx
    Y = (v - cy) * Z / fy
    point_cloud = torch.cat((X, Y, Z), dim=0).permute(1, 2, 0)
    x = torch.arange(W, dtype=torch.float32).view(1, W).repeat(H, 1)
    y = torch.arange(H, dtype=torch.float32).view(H, 1).repeat(1, W)
    xy1 = torch.stack((x, y, torch.ones((H, W)))).view(3, -1).double()
    k_inv_dot_xy1 = torch.matmul(intrinsic_inv, xy1)
    N = masks.shape[0]
    planes = torch.full((N, 4), float("nan"), dtype=torch.float64)
    valid = torch.zeros(N, dtype=torch.bool)
    out = depth.clone()
    for i in range(N):
        pts = point_cloud[masks[i], :]
        if pts.shape[0] < 3:
            continue
        center = pts.mean(dim=0)
        adj = pts - center
        U, S, _ = torch.svd(torch.mm(adj.transpose(0, 1), adj))
        if not bool(S[1] > 1e-12 * S[0]):
            continue
        normal = U[:, 2]
        plane_depth = (torch.dot(center, normal) / torch.matmul(normal, k_inv_dot_xy1)).view(H, W)
        out = torch.where(masks[i], plane_depth.float(), out)
        d = torch.dot(center, normal)
        sign = -1.0 if d < 0 else 1.0
        planes[i, :3], planes[i, 3] = normal * sign, d * sign
        valid[i] = True
    out = out.numpy().copy()
    if depth_range is not None:
        out[out <= depth_range[0]] = np.nan
        out[out >= depth_range[1]] = np.nan
    return out, planes, valid


def plane_depth_map(n, d, k_matrix, H, W):
    """fp64 [H,W] depth of the plane n . X = d seen through K (the ray of pixel (v, u) is K^-1 [u, v, 1])"""
    kinv = np.linalg.inv(np.asarray(k_matrix, np.float64))
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    r = np.einsum("ij,jhw->ihw", kinv, np.stack([u, v, np.ones_like(u)]))
    return d / np.einsum("i,ihw->hw", np.asarray(n, np.float64), r)


def k_of(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
