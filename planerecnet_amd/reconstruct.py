"""The reconstruction itself: the triangle mesh and the point cloud of a depth map, and their PLY files (include/prn.h: prn_mesh; DESIGN.md
section 22).

planes.planar_depth gives depth that is flat under every valid instance, plane_eval.label_map the owner of every pixel; `mesh` turns
(depth, labels, K) into vertices and triangles where they are -- on the device -- so what travels is the model, not H x W maps:

  valid pixel  z finite and lo < z < hi in fp32 (depth_range, default (0, inf)); with planar_only also label > 0
  vertex       one per valid pixel, id = the valid pixels before it in row-major order of its image; X = ((double)u - cx) * z / fx,
               Y = ((double)v - cy) * z / fy, Z = z (fp64 in this order, rounded to fp32 once; u, v integer pixel indices, K as in planes);
               it carries the pixel's label and colour
  triangles    the quad a = (v,u), b = (v+1,u), c = (v,u+1), d = (v+1,u+1) gives t0 = (a,b,c) and t1 = (c,b,d), both facing the camera (image
               y down, camera looking along +Z: n . p < 0).  One is emitted iff its three pixels are valid, carry one label (same_label) and
               zmax - zmin <= max_gap * zmin (relative) or <= max_gap, subtraction and product each rounded to fp32.  Faces are row-major by
               quad, t0 before t1, and hold vertex ids

Everything that decides placement is an integer, so the outputs are specified bit for bit.  Device tensors run on the device (four
launches whatever the batch, no host synchronisation, inputs untouched: sizes are capacities, the counts stay on the device), CPU tensors
on the host in numpy with the same outputs bit for bit -- the rule of morphology.erode and plane_eval.label_map.
"""
import math
import numbers

import numpy as np
import torch

from ._masks import _bytes_buffer, _describe, _p, _stream

__all__ = ["mesh", "point_cloud", "Mesh", "write_ply", "read_ply", "reconstruct_results", "results_depth_labels", "block_pixels", "scan_chunk", "MAX_PIXELS"]

MAX_PIXELS = 1 << 24               # H * W stays below this
RELATIVE, SAME_LABEL, PLANAR_ONLY, FACES = 1, 2, 4, 8      # include/prn.h: PRN_MESH_*
_MAX_BATCH = 65535                 # images per library call (the grid's y)


def block_pixels():
    """consecutive pixels one workgroup of the device path counts and places (prn_mesh_block_pixels)"""
    from ._lib import lib
    return int(lib.prn_mesh_block_pixels())


def scan_chunk():
    """workgroups one step of the per-image scan takes (prn_mesh_scan_chunk)"""
    from ._lib import lib
    return int(lib.prn_mesh_scan_chunk())


class Mesh:
    """What `mesh` returns, at capacity (cap = H W vertices, capf = 2 (H-1) (W-1) faces an image); rows past the counts are unspecified.
      vertices [B,cap,3] fp32   labels [B,cap] int32   colors [B,cap,3] uint8 or None   faces [B,capf,3] int32 or None (point cloud)
      counts [B,2] int32 = (vertices, faces) of each image   vertex_id [B,H,W] int32: a pixel's vertex id, -1 where it is invalid
      normals [B,cap,3] fp32 or None: each vertex's pixel's normal, where `mesh` was given a normal map"""
    __slots__ = ("vertices", "labels", "colors", "faces", "counts", "vertex_id", "normals")

    def __init__(self, vertices, labels, colors, faces, counts, vertex_id, normals=None):
        self.vertices, self.labels, self.colors, self.faces, self.counts, self.vertex_id = vertices, labels, colors, faces, counts, vertex_id
        self.normals = normals

    def cpu(self):
        """-> one dict per image: "vertices" [Nv,3] float32, "faces" [Nf,3] int32 or None, "labels" [Nv] int32, "colors" [Nv,3] uint8 or None, as
        numpy arrays trimmed to the counts, and "normals" [Nv,3] float32 only where the mesh has them.  Two downloads at most: the counts, then
        the trimmed ranges of every array in one buffer."""
        counts = self.counts.cpu().numpy()
        fields = [("vertices", self.vertices, 0), ("faces", self.faces, 1), ("labels", self.labels, 0), ("colors", self.colors, 0)]
        if self.normals is not None:
            fields.append(("normals", self.normals, 0))
        parts, plan = [], []
        for b in range(counts.shape[0]):
            for name, t, which in fields:
                if t is None:
                    plan.append((b, name, None, None, 0))
                    continue
                part = t[b, :int(counts[b, which])]
                parts.append(part.reshape(-1).view(torch.uint8))
                plan.append((b, name, part.dtype, tuple(part.shape), part.numel() * part.element_size()))
        flat = (torch.cat(parts) if parts else torch.zeros(0, dtype=torch.uint8)).cpu().numpy()
        out, o = [{} for _ in range(counts.shape[0])], 0
        for b, name, dtype, shape, nbytes in plan:
            if dtype is None:
                out[b][name] = None
                continue
            np_dtype = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}[dtype]
            out[b][name] = flat[o:o + nbytes].view(np_dtype).reshape(shape).copy()
            o += nbytes
        return out


# ---- host path (numpy) -----------------------------------------------------------------------------------------------------------

def _mesh_np(z, lab, col, k, lo, hi, gap, relative, same_label, planar_only, faces):
    """one image: z [H,W] float32, lab [H,W] int32, col [H,W,3] uint8 or None, k [9] float64 -> (vertices, labels, colors, faces, id map)"""
    H, W = z.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        valid = np.isfinite(z) & (z > lo) & (z < hi)
        if planar_only:
            valid &= lab > 0
        flat = valid.reshape(-1)
        vid = np.where(flat, np.cumsum(flat, dtype=np.int64) - 1, -1).astype(np.int32).reshape(H, W)
        v, u = np.nonzero(valid)
        zz = z[valid].astype(np.float64)
        pos = np.stack([(u.astype(np.float64) - k[2]) * zz / k[0], (v.astype(np.float64) - k[5]) * zz / k[4], zz], 1).astype(np.float32)
        tri = None
        if faces:
            c = [(slice(0, H - 1), slice(0, W - 1)), (slice(1, H), slice(0, W - 1)), (slice(0, H - 1), slice(1, W)), (slice(1, H), slice(1, W))]   # a b c d
            keep, ids = [], []
            for t in ((0, 1, 2), (2, 1, 3)):
                zs, ls, ok = [z[c[i]] for i in t], [lab[c[i]] for i in t], valid[c[t[0]]] & valid[c[t[1]]] & valid[c[t[2]]]
                if same_label:
                    ok = ok & (ls[0] == ls[1]) & (ls[1] == ls[2])
                zmax, zmin = np.maximum(np.maximum(zs[0], zs[1]), zs[2]), np.minimum(np.minimum(zs[0], zs[1]), zs[2])
                keep.append(ok & ((zmax - zmin) <= (gap * zmin if relative else gap)))
                ids.append(np.stack([vid[c[i]] for i in t], -1))
            tri = np.stack(ids, 2)[np.stack(keep, 2)].astype(np.int32).reshape(-1, 3)                  # [H-1,W-1,2,3] under [H-1,W-1,2]: row-major, t0 first
    return pos, lab[valid], None if col is None else col[valid], tri, vid


# ---- mesh ------------------------------------------------------------------------------------------------------------------------

def _check_inputs(depth, labels, colors, depth_range, max_gap, what):
    if not (torch.is_tensor(depth) and depth.dtype == torch.float32 and
            (depth.dim() == 2 or (depth.dim() == 3 and depth.shape[0] == 1) or (depth.dim() == 4 and depth.shape[1] == 1))):
        raise RuntimeError("%s: depth must be a [H,W], [1,H,W] or [B,1,H,W] fp32 tensor, got %s" % (what, _describe(depth)))
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    B = int(depth.shape[0]) if depth.dim() == 4 else 1
    if B < 1 or H < 1 or W < 1:
        raise RuntimeError("%s: depth %s holds no pixel" % (what, tuple(depth.shape)))
    if H * W >= MAX_PIXELS:
        raise RuntimeError("%s: H * W must be below 2^24, got %d x %d" % (what, H, W))
    if labels is not None and not (torch.is_tensor(labels) and labels.dtype == torch.int32 and labels.device == depth.device and
                                   tuple(labels.shape) in ((B, H, W),) + (((H, W),) if B == 1 else ())):
        raise RuntimeError("%s: labels must be an int32 [H,W] or [B,H,W] tensor (B=%d H=%d W=%d) on %s, got %s" % (what, B, H, W, depth.device, _describe(labels)))
    if colors is not None and not (torch.is_tensor(colors) and colors.dtype == torch.uint8 and colors.device == depth.device and
                                   tuple(colors.shape) in ((B, H, W, 3),) + (((H, W, 3),) if B == 1 else ())):
        raise RuntimeError("%s: colors must be a uint8 [H,W,3] or [B,H,W,3] tensor (B=%d H=%d W=%d) on %s, got %s" % (what, B, H, W, depth.device, _describe(colors)))
    if isinstance(max_gap, bool) or not isinstance(max_gap, numbers.Real) or not 0 <= float(max_gap) < 3.4028235677973366e38:      # (the first double that rounds to fp32 inf)
        raise ValueError("%s: max_gap must be a finite number >= 0 (as fp32), got %r" % (what, max_gap))
    try:
        lo, hi = (float(v) for v in depth_range)
    except (TypeError, ValueError):
        raise ValueError("%s: depth_range must be a pair of numbers (lo, hi), got %r" % (what, depth_range))
    if math.isnan(lo) or math.isnan(hi):
        raise ValueError("%s: depth_range must not hold NaN, got %r" % (what, depth_range))
    return B, H, W, np.float32(lo), np.float32(hi), np.float32(max_gap)


def _intrinsics_np(k_matrix, B):
    k = np.asarray(k_matrix.detach().cpu() if torch.is_tensor(k_matrix) else k_matrix, dtype=np.float64)
    if k.shape not in ((3, 3), (B, 3, 3)):
        raise RuntimeError("k_matrix must be [3,3] or [B,3,3] (B=%d), got %s" % (B, tuple(k.shape)))
    return np.broadcast_to(k, (B, 3, 3)).reshape(B, 9)


@torch.no_grad()
def mesh(depth, k_matrix, labels=None, colors=None, depth_range=(0.0, math.inf), max_gap=0.05, relative=True, same_label=True, planar_only=False,
         faces=True, normals=None):
    """The triangle mesh of a depth map (module docstring for the rules).

    depth        [H,W], [1,H,W] or [B,1,H,W] fp32; H * W < 2^24
    k_matrix     intrinsics K, [3,3] or [B,3,3] (tensor anywhere, or an array)
    labels       int32 [H,W] or [B,H,W] on depth's device (plane_eval.label_map's output); None = all 0
    colors       uint8 [H,W,3] or [B,H,W,3] on depth's device, copied to the vertices in the order given; None = no colours
    depth_range  (lo, hi): a pixel is valid iff its depth is finite and lo < z < hi
    max_gap      the largest depth spread of a triangle's corners: a fraction of their smallest depth (relative) or metres; finite, >= 0
    same_label   a triangle's corners carry one label        planar_only   only pixels with label > 0 are valid
    faces        False: the point cloud alone -- no face pass, Mesh.faces is None and counts[:, 1] is 0
    normals      fp32 [H,W,3] or [B,H,W,3] on depth's device (normals.from_depth's map): Mesh.normals holds each vertex's pixel's row
    -> Mesh, on depth's device.  Nothing is read back: the arrays have capacity size and the counts say how much of them is written."""
    what = "mesh"
    B, H, W, lo, hi, gap = _check_inputs(depth, labels, colors, depth_range, max_gap, what)
    dev = depth.device
    if normals is not None and not (torch.is_tensor(normals) and normals.dtype == torch.float32 and normals.device == dev and
                                    tuple(normals.shape) in ((B, H, W, 3),) + (((H, W, 3),) if B == 1 else ())):
        raise RuntimeError("%s: normals must be an fp32 [H,W,3] or [B,H,W,3] tensor (B=%d H=%d W=%d) on %s, got %s" % (what, B, H, W, dev, _describe(normals)))
    cap, capf = H * W, 2 * (H - 1) * (W - 1)
    z = depth.detach().reshape(B, H, W).contiguous()
    lab = None if labels is None else labels.reshape(B, H, W).contiguous()
    col = None if colors is None else colors.reshape(B, H, W, 3).contiguous()
    if not z.is_cuda:
        if dev.type != "cpu":
            raise RuntimeError("%s: depth must be a device or a CPU tensor, got %s" % (what, _describe(depth)))
        k = _intrinsics_np(k_matrix, B)
        zn, ln = z.numpy(), np.zeros((B, H, W), np.int32) if lab is None else lab.numpy()
        out = Mesh(torch.zeros(B, cap, 3), torch.zeros(B, cap, dtype=torch.int32), None if col is None else torch.zeros(B, cap, 3, dtype=torch.uint8),
                   torch.zeros(B, capf, 3, dtype=torch.int32) if faces else None, torch.zeros(B, 2, dtype=torch.int32),
                   torch.zeros(B, H, W, dtype=torch.int32))
        for b in range(B):
            pos, vl, vc, tri, vid = _mesh_np(zn[b], ln[b], None if col is None else col[b].numpy(), k[b], lo, hi, gap, relative, same_label, planar_only, faces)
            nv = pos.shape[0]
            out.vertices[b, :nv] = torch.from_numpy(pos)
            out.labels[b, :nv] = torch.from_numpy(np.ascontiguousarray(vl))
            if vc is not None:
                out.colors[b, :nv] = torch.from_numpy(np.ascontiguousarray(vc))
            if faces:
                out.faces[b, :tri.shape[0]] = torch.from_numpy(tri)
                out.counts[b, 1] = tri.shape[0]
            out.counts[b, 0] = nv
            out.vertex_id[b] = torch.from_numpy(vid)
        out.normals = _vertex_rows(normals, out.vertex_id)
        return out
    from ._lib import check, lib
    from .planes import _intrinsics
    k = _intrinsics(k_matrix, B, dev)
    out = Mesh(torch.empty(B, cap, 3, dtype=torch.float32, device=dev), torch.empty(B, cap, dtype=torch.int32, device=dev),
               None if col is None else _bytes_buffer(B * cap * 3, dev).view(B, cap, 3),
               torch.empty(B, capf, 3, dtype=torch.int32, device=dev) if faces else None, torch.empty(B, 2, dtype=torch.int32, device=dev),
               torch.empty(B, H, W, dtype=torch.int32, device=dev))
    flags = (RELATIVE if relative else 0) | (SAME_LABEL if same_label else 0) | (PLANAR_ONLY if planar_only else 0) | (FACES if faces else 0)
    stream = _stream(dev)
    for b0 in range(0, B, _MAX_BATCH):
        n = min(B, b0 + _MAX_BATCH) - b0
        ws = torch.empty(lib.prn_mesh_ws_bytes(n, H, W) // 4, dtype=torch.int32, device=dev)
        check(lib.prn_mesh(_p(z[b0:]), None if lab is None else _p(lab[b0:]), None if col is None else _p(col[b0:]), _p(k[b0:]), n, H, W, float(lo), float(hi),
                           float(gap), flags, _p(ws), _p(out.vertices[b0:]), _p(out.labels[b0:]), None if col is None else _p(out.colors[b0:]),
                           _p(out.vertex_id[b0:]), _p(out.faces[b0:]) if faces and capf else None, _p(out.counts[b0:]), stream), "prn_mesh")
        del ws                                                       # (stream-ordered allocator: reuse after this point is ordered behind the launches)
    out.normals = _vertex_rows(normals, out.vertex_id)
    return out


def _vertex_rows(pixel_map, vertex_id):
    """a per-pixel map [B,H,W,3] (or [H,W,3], B = 1) -> its rows in vertex order [B,cap,3]: a scatter through the id map in tensor ops on the
    map's device (no synchronisation; invalid pixels go to a row past the capacity that is cut off); rows past the counts are zero"""
    if pixel_map is None:
        return None
    B, H, W = vertex_id.shape
    cap = H * W
    idx = vertex_id.reshape(B, cap).long()
    idx = torch.where(idx < 0, torch.full_like(idx, cap), idx)
    rows = torch.zeros(B, cap + 1, 3, dtype=pixel_map.dtype, device=pixel_map.device)
    rows.scatter_(1, idx[..., None].expand(B, cap, 3), pixel_map.detach().reshape(B, cap, 3))
    return rows[:, :cap].contiguous()


def point_cloud(depth, k_matrix, labels=None, colors=None, depth_range=(0.0, math.inf), planar_only=False, normals=None):
    """The point cloud alone: `mesh` with faces=False (one vertex per valid pixel, no face pass)."""
    return mesh(depth, k_matrix, labels=labels, colors=colors, depth_range=depth_range, planar_only=planar_only, faces=False, normals=normals)


# ---- from the network's results --------------------------------------------------------------------------------------------------------

@torch.no_grad()
def results_depth_labels(results):
    """per-image result dicts -> (depth [B,1,H,W] fp32, labels [B,H,W] int32): what reconstruct_results meshes (its docstring)"""
    from . import plane_eval
    depth = torch.cat([(r["pred_plane_depth"] if r.get("pred_plane_depth") is not None else r["pred_depth"]).reshape(1, 1, *r["pred_depth"].shape[-2:])
                       for r in results]).float()
    B, _, H, W = depth.shape
    masks = []
    for r in results:
        m = r.get("pred_plane_masks") if r.get("pred_plane_masks") is not None else r.get("pred_masks")
        if m is not None and m.dtype not in (torch.bool, torch.uint8):
            m = m != 0
        masks.append(None if m is None or m.shape[0] == 0 else m)
    if any(m is not None for m in masks):
        return depth, plane_eval.label_map(masks, "last")
    return depth, torch.zeros(B, H, W, dtype=torch.int32, device=depth.device)


@torch.no_grad()
def reconstruct_results(results, k_matrix, frames=None, normals=None, **mesh_kwargs):
    """The mesh of planes.planar_depth's (or the network's) per-image result dicts, as one batch.
      depth    "pred_plane_depth" where a dict has it, else "pred_depth"
      labels   plane_eval.label_map(masks, "last") of "pred_plane_masks" where present, else "pred_masks" -- the owner of every pixel in
               the order planar_depth paints; an image without detections has label 0 everywhere
      colours  frames: None, a uint8 [B,H,W,3] tensor / array, or a list of B [H,W,3] ones (moved to the depth's device)
      normals  None, or a dict of normals.from_depth keywords ({} = its defaults): the normals of the depth and labels that are meshed
               go to the vertices (Mesh.normals)
    mesh_kwargs go to `mesh`.  -> Mesh"""
    depth, labels = results_depth_labels(results)
    dev = depth.device
    colors = None
    if frames is not None:
        if isinstance(frames, (list, tuple)):
            frames = torch.stack([torch.as_tensor(f) for f in frames])
        colors = torch.as_tensor(frames).to(dev)
    if normals is not None:
        from . import normals as _normals
        normals = _normals.from_depth(depth, k_matrix, labels=labels, **dict(normals))[0]
    return mesh(depth, k_matrix, labels=labels, colors=colors, normals=normals, **mesh_kwargs)


# ---- PLY -------------------------------------------------------------------------------------------------------------------------

_FORMATS = {True: "binary_little_endian", False: "ascii"}


def _vertex_dtype(with_colors, with_normals=False):
    return np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if with_normals else []) +
                    ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if with_colors else []) + [("label", "<i4")])


_FACE_DTYPE = np.dtype([("n", "u1"), ("ids", "<i4", (3,))])


_NORMAL_LINES = ["property float nx", "property float ny", "property float nz"]


def _header(binary, comments, nv, with_colors, nf, with_normals=False):
    lines = ["ply", "format %s 1.0" % _FORMATS[bool(binary)]] + ["comment " + c for c in comments] + ["element vertex %d" % nv]
    lines += ["property float x", "property float y", "property float z"]
    if with_normals:
        lines += _NORMAL_LINES
    if with_colors:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    lines += ["property int label"]
    if nf is not None:
        lines += ["element face %d" % nf, "property list uchar int vertex_indices"]
    return "\n".join(lines + ["end_header"]) + "\n"


def write_ply(path, image_dict, binary=True, comment=None):
    """Writes one image's mesh (an entry of Mesh.cpu(): "vertices" [Nv,3] float32, "labels" [Nv] int32, "colors" [Nv,3] uint8 or None,
    "faces" [Nf,3] int32 or None) as a PLY file: binary little-endian or ascii (floats with nine significant digits: they read back
    exactly).  comment: a string or a list of strings, one `comment` line each.  Colour properties and the face element are written only
    where the dict has them, and `property float nx|ny|nz` directly after z where it has "normals" [Nv,3] float32 (Mesh.cpu() of a mesh with
    normals); a dict without them gives the file it always gave."""
    vertices = np.ascontiguousarray(image_dict["vertices"], dtype=np.float32).reshape(-1, 3)
    nv = vertices.shape[0]
    labels = np.asarray(image_dict["labels"], dtype=np.int32).reshape(-1)
    colors = None if image_dict.get("colors") is None else np.asarray(image_dict["colors"], dtype=np.uint8).reshape(-1, 3)
    faces = None if image_dict.get("faces") is None else np.asarray(image_dict["faces"], dtype=np.int32).reshape(-1, 3)
    normals = None if image_dict.get("normals") is None else np.ascontiguousarray(image_dict["normals"], dtype=np.float32).reshape(-1, 3)
    if labels.shape[0] != nv or (colors is not None and colors.shape[0] != nv) or (normals is not None and normals.shape[0] != nv):
        raise ValueError("write_ply: %d vertices, %d labels, %s colours, %s normals" % (nv, labels.shape[0], "no" if colors is None else colors.shape[0],
                                                                                      "no" if normals is None else normals.shape[0]))
    comments = [] if comment is None else ([comment] if isinstance(comment, str) else list(comment))
    if any("\n" in c or "\r" in c for c in comments):
        raise ValueError("write_ply: a comment must be one line")
    head = _header(binary, comments, nv, colors is not None, None if faces is None else faces.shape[0], normals is not None).encode("ascii")
    with open(path, "wb") as f:
        f.write(head)
        if binary:
            rec = np.empty(nv, _vertex_dtype(colors is not None, normals is not None))
            rec["x"], rec["y"], rec["z"], rec["label"] = vertices[:, 0], vertices[:, 1], vertices[:, 2], labels
            if normals is not None:
                rec["nx"], rec["ny"], rec["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
            if colors is not None:
                rec["red"], rec["green"], rec["blue"] = colors[:, 0], colors[:, 1], colors[:, 2]
            f.write(rec.tobytes())
            if faces is not None:
                fr = np.empty(faces.shape[0], _FACE_DTYPE)
                fr["n"], fr["ids"] = 3, faces
                f.write(fr.tobytes())
        else:
            rows = []
            for i in range(nv):
                row = "%.9g %.9g %.9g" % tuple(float(x) for x in vertices[i])
                if normals is not None:
                    row += " %.9g %.9g %.9g" % tuple(float(x) for x in normals[i])
                if colors is not None:
                    row += " %d %d %d" % tuple(int(x) for x in colors[i])
                rows.append(row + " %d" % int(labels[i]))
            if faces is not None:
                rows += ["3 %d %d %d" % tuple(int(x) for x in t) for t in faces]
            f.write(("\n".join(rows) + ("\n" if rows else "")).encode("ascii"))


def _bad(path, why):
    return ValueError("read_ply: %s is not a file write_ply made: %s" % (path, why))


def read_ply(path):
    """Reads back exactly the files write_ply makes (anything else: ValueError) -> the dict write_ply took ("vertices", "faces", "labels",
    "colors"; faces / colors None where the file has none; "normals" only where the file has them) plus "comments": the list of comment
    strings."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise _bad(path, "no end_header line")
    try:
        lines = data[:end].decode("ascii").split("\n")[:-1] + ["end_header"]
    except UnicodeDecodeError:
        raise _bad(path, "the header is not ascii")
    body = data[end + len(b"end_header\n"):]
    if len(lines) < 3 or lines[0] != "ply" or lines[1] not in ("format binary_little_endian 1.0", "format ascii 1.0"):
        raise _bad(path, "the first lines are not `ply` and a known `format`")
    binary = lines[1].startswith("format binary")
    i, comments = 2, []
    while lines[i].startswith("comment "):
        comments.append(lines[i][len("comment "):])
        i += 1

    def count(line, prefix):
        if not line.startswith(prefix) or not line[len(prefix):].isdigit():
            raise _bad(path, "expected `%sN`, got %r" % (prefix, line))
        return int(line[len(prefix):])
    nv = count(lines[i], "element vertex ")
    rest = lines[i + 1:]
    with_normals = rest[3:6] == _NORMAL_LINES
    o = 6 if with_normals else 3                                    # cells of a vertex before its colours
    with_colors = rest[o:o + 3] == ["property uchar red", "property uchar green", "property uchar blue"]
    nf = None
    tail = rest[o + (4 if with_colors else 1):]
    if len(tail) == 3:
        nf = count(tail[0], "element face ")
    if "".join(l + "\n" for l in lines) != _header(binary, comments, nv, with_colors, nf, with_normals):
        raise _bad(path, "the header differs from the one write_ply writes")
    vdt = _vertex_dtype(with_colors, with_normals)
    if binary:
        need = nv * vdt.itemsize + (0 if nf is None else nf * _FACE_DTYPE.itemsize)
        if len(body) != need:
            raise _bad(path, "%d bytes after the header, %d expected" % (len(body), need))
        rec = np.frombuffer(body, vdt, nv)
        vertices = np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32) if nv else np.zeros((0, 3), np.float32)
        normals = (np.stack([rec["nx"], rec["ny"], rec["nz"]], 1).astype(np.float32) if nv else np.zeros((0, 3), np.float32)) if with_normals else None
        labels = rec["label"].astype(np.int32)
        colors = np.stack([rec["red"], rec["green"], rec["blue"]], 1).astype(np.uint8) if with_colors else None
        faces = None
        if nf is not None:
            fr = np.frombuffer(body, _FACE_DTYPE, nf, nv * vdt.itemsize)
            if (fr["n"] != 3).any():
                raise _bad(path, "a face that is no triangle")
            faces = fr["ids"].astype(np.int32).reshape(-1, 3)
    else:
        try:
            rows = body.decode("ascii").split("\n")
        except UnicodeDecodeError:
            raise _bad(path, "the body is not ascii")
        if rows[-1] != "" or len(rows) - 1 != nv + (nf or 0):
            raise _bad(path, "%d complete lines after the header, %d expected" % (len(rows) - 1, nv + (nf or 0)))
        width = o + (4 if with_colors else 1)
        try:
            cells = [r.split(" ") for r in rows[:-1]]
            if any(len(c) != width for c in cells[:nv]) or any(len(c) != 4 or c[0] != "3" for c in cells[nv:]):
                raise ValueError
            vertices = np.array([[float(x) for x in c[:3]] for c in cells[:nv]], dtype=np.float64).reshape(-1, 3).astype(np.float32)
            normals = np.array([[float(x) for x in c[3:6]] for c in cells[:nv]], dtype=np.float64).reshape(-1, 3).astype(np.float32) if with_normals else None
            labels = np.array([int(c[-1]) for c in cells[:nv]], dtype=np.int64)
            colors = np.array([[int(x) for x in c[o:o + 3]] for c in cells[:nv]], dtype=np.int64).reshape(-1, 3) if with_colors else None
            faces = np.array([[int(x) for x in c[1:]] for c in cells[nv:]], dtype=np.int64).reshape(-1, 3) if nf is not None else None
        except ValueError:
            raise _bad(path, "a malformed line in the body")
        if (colors is not None and ((colors < 0) | (colors > 255)).any()) or (np.abs(labels) >= 2 ** 31).any() or (faces is not None and (np.abs(faces) >= 2 ** 31).any()):
            raise _bad(path, "a value outside its property's type")
        labels = labels.astype(np.int32)
        colors = None if colors is None else colors.astype(np.uint8)
        faces = None if faces is None else faces.astype(np.int32)
    if faces is not None and faces.size and (faces.min() < 0 or faces.max() >= nv):
        raise _bad(path, "a face refers to a vertex the file does not hold")
    out = {"vertices": vertices, "faces": faces, "labels": labels, "colors": colors, "comments": comments}
    if with_normals:
        out["normals"] = normals
    return out
