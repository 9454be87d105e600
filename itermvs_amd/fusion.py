"""Depth-map filtering and fusion after inference (the reference's ``filter_depth``, eval.py:215-309) on the GPU:
one ``itermvs_fuse_depth`` launch per reference view instead of ~40 full-frame numpy passes per (reference, source)
pair.  Host side: the text formats of a scan folder (``pair.txt``, ``cams_1/*_cam.txt``, eval.py:56-65,90-100), PFM
depth / confidence maps (datasets/data_io.py) and the fused point cloud as a binary little-endian PLY with the vertex
layout of eval.py:298-308 (x, y, z float32; red, green, blue uint8)."""
from __future__ import annotations

import contextlib
import os
import time
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .data_io import read_pfm


def read_camera_parameters(filename: str) -> Tuple[np.ndarray, np.ndarray]:
    """eval.py:56-65 -> (intrinsics [3,3], extrinsics [4,4]) float32"""
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape((4, 4))
    intrinsics = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape((3, 3))
    return intrinsics, extrinsics


def read_pair_file(filename: str) -> List[Tuple[int, List[int]]]:
    """eval.py:90-100"""
    data = []
    with open(filename) as f:
        num_viewpoint = int(f.readline())
        for _ in range(num_viewpoint):
            ref_view = int(f.readline().rstrip())
            src_views = [int(x) for x in f.readline().rstrip().split()[1::2]]
            if len(src_views) != 0:
                data.append((ref_view, src_views))
    return data


def pair_matrices(k_ref: np.ndarray, e_ref: np.ndarray, k_src: np.ndarray, e_src: np.ndarray) -> np.ndarray:
    """the six float32 matrices of one (reference, source) pair in itermvs_fuse_depth's [60] layout, inverted and
    composed with numpy in float32 exactly as eval.py:162-189 does"""
    t_rs = np.matmul(e_src, np.linalg.inv(e_ref))
    t_sr = np.matmul(e_ref, np.linalg.inv(e_src))
    parts = [np.linalg.inv(k_ref), t_rs[:3], k_src, np.linalg.inv(k_src), t_sr[:3], k_ref]
    return np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in parts])


def fuse_reference_view(depth_ref, conf_ref, k_ref, e_ref, src_depths: Sequence, src_ks: Sequence, src_es: Sequence,
                        geo_pixel_thres=1.0, geo_depth_thres=0.01, photo_thres=0.3, geo_mask_thres=3, device="cuda"):
    """eval.py:238-269 for one reference view (numpy or torch inputs) -> torch tensors
    (depth_est_averaged float64, photo_mask, geo_mask, final_mask uint8, geo_mask_sum int32)"""
    dev = torch.device(device)
    as_t = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, torch.float32)
    mats = np.stack([pair_matrices(np.asarray(k_ref), np.asarray(e_ref), np.asarray(k), np.asarray(e))
                     for k, e in zip(src_ks, src_es)])
    return ops.fuse_depth(as_t(depth_ref), as_t(conf_ref), [as_t(d) for d in src_depths], torch.from_numpy(mats).to(dev),
                          geo_pixel_thres, geo_depth_thres, photo_thres, geo_mask_thres)


def ply_header(n: int, normals: bool = False) -> bytes:
    """the header of the binary little-endian PLY with ``n`` vertices of eval.py:298-308; ``normals``: with nx, ny, nz between
    z and red, the property order of COLMAP's fused.ply"""
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "%sproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
            % (n, "property float nx\nproperty float ny\nproperty float nz\n" if normals else "")).encode("ascii")


def write_ply(filename: str, xyz: np.ndarray, rgb: np.ndarray) -> None:
    """binary little-endian PLY, vertex = (x, y, z float32, red, green, blue uint8) -- the element eval.py:298-308 builds"""
    n = xyz.shape[0]
    v = np.empty(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    with open(filename, "wb") as f:
        f.write(ply_header(n))
        f.write(v.tobytes())


def read_scan_image(filename: str, img_wh: Tuple[int, int], want_pixels: bool = True, as_uint8: bool = False):
    """eval.py:68-74 ``read_img``: -> (RGB float32 [H,W,3] in 0..1 resized to ``img_wh`` or None, original_h, original_w);
    ``as_uint8``: the resized pixels as PIL holds them, before the division (what the device path of the fusion uploads).
    The reference resizes with ``cv2.resize(INTER_LINEAR)``; cv2 is not a dependency here, PIL's bilinear filter takes its
    place (vertex colours only -- the geometry never reads the pixels)."""
    from PIL import Image
    with Image.open(filename) as im:
        original_w, original_h = im.size
        px = None
        if want_pixels:
            im = im.convert("RGB")
            if (original_w, original_h) != tuple(img_wh):
                im = im.resize(tuple(img_wh), Image.BILINEAR)
            px = np.array(im, dtype=np.uint8) if as_uint8 else np.asarray(im, dtype=np.float32) / 255.0
    return px, original_h, original_w


def save_mask(filename: str, mask) -> None:
    """eval.py:79-82 ``save_mask``: a boolean map as an 8-bit image of 0 / 255"""
    from PIL import Image
    Image.fromarray(np.asarray(mask).astype(bool).astype(np.uint8) * 255).save(filename)


def _save_view_masks(mask_folder: str, view: int, photo, geo, final) -> None:
    """eval.py:266-269: mask/<view>_photo.png, _geo.png, _final.png"""
    os.makedirs(mask_folder, exist_ok=True)
    for name, m in (("photo", photo), ("geo", geo), ("final", final)):
        save_mask(os.path.join(mask_folder, "{:0>8}_{}.png".format(view, name)), m.cpu().numpy() if torch.is_tensor(m) else m)


def group_views(n_views: int, h: int, w: int, budget_bytes: int, record_bytes: int = ops.POINT_RECORD_BYTES) -> List[Tuple[int, int]]:
    """consecutive [start, stop) ranges of reference views whose worst case (every pixel of every view survives:
    views * h * w * record_bytes, 15 bytes per vertex unless given) fits ``budget_bytes``; a budget below one view cannot be met"""
    per_view = h * w * record_bytes
    k = int(budget_bytes) // per_view
    if k < 1:
        raise ValueError(f"records budget of {budget_bytes} bytes is below one {w}x{h} view ({per_view} bytes)")
    return [(i, min(i + k, n_views)) for i in range(0, n_views, k)]


DOWNLOAD_CHUNK_BYTES = 32 << 20


@contextlib.contextmanager
def _remove_on_error(filename: str):
    """no half-written point cloud stays behind when the fusion raises"""
    try:
        yield
    except BaseException:
        if os.path.exists(filename):
            os.remove(filename)
        raise


def _download(records: torch.Tensor, nbytes: int, write, seconds: Dict[str, float]) -> int:
    """records[:nbytes] -> ``write(uint8 numpy view)`` in order, through two pinned staging buffers: the copy of chunk i + 1
    runs while chunk i is written.  -> number of chunks"""
    if nbytes == 0:
        return 0
    chunk = min(DOWNLOAD_CHUNK_BYTES, nbytes)
    pin = [torch.empty(chunk, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    done = [torch.cuda.Event(), torch.cuda.Event()]
    n_chunks = (nbytes + chunk - 1) // chunk
    size = lambda i: min(chunk, nbytes - i * chunk)    # noqa: E731

    def issue(i):
        pin[i % 2][:size(i)].copy_(records[i * chunk:i * chunk + size(i)], non_blocking=True)
        done[i % 2].record()

    issue(0)
    for i in range(n_chunks):
        if i + 1 < n_chunks:
            issue(i + 1)                               # its buffer was written out in the previous turn
        t0 = time.perf_counter()
        done[i % 2].synchronize()
        t1 = time.perf_counter()
        write(pin[i % 2][:size(i)].numpy())
        seconds["download_wait"] += t1 - t0
        seconds["file_write"] += time.perf_counter() - t1
    return n_chunks


def fuse_scan(pairs: Sequence[Tuple[int, Sequence[int]]], cams, depths, confidences, images, plyfilename: str,
              geo_pixel_thres: float, geo_depth_thres: float, photo_thres: float, geo_mask_thres: int = 3, device: str = "cuda",
              records_budget: int = 2 << 30, mask_folder: str = None, group_capacity: int = None,
              info: dict = None, dedupe: bool = False, normals: bool = False,
              normal_edge_thres: float = 0.01) -> Dict[int, Tuple[float, float, float]]:
    """eval.py:215-309 for a scan that is already in memory, with the point cloud assembled on the GPU: per reference view one
    ``itermvs_fuse_depth`` and one ``itermvs_fuse_points``, enqueued back to back; the host synchronises once per GROUP of
    reference views, downloads the group's finished vertex records and appends them to the PLY.

    pairs: as ``read_pair_file`` returns them; cams[view] = (K [3,3], E [4,4]) already rescaled to the depth maps' size;
    depths[view], confidences[ref_view]: [H,W] maps, images[ref_view]: uint8 [H,W,3] (numpy or torch, either device).
    records_budget: bytes of GPU memory for the vertex records; the reference views are grouped (``group_views``) so that a
    group fits even if every pixel survives.  group_capacity: vertices the buffer holds instead of that worst case (a group
    that emits more raises).  mask_folder: write the three masks of every reference view there (eval.py:266-269).
    info: filled with the groups, the number of synchronisations / downloads and where the time went.
    dedupe: emit each surface point once per scan (``itermvs_fuse_depth_claim`` in place of ``itermvs_fuse_depth``): one zeroed
    uint8 [H,W] claim map per view lives on the GPU for the whole scan, across the flush groups; a pixel that an emitted point of an
    earlier reference view was verified against is left out of ``final``.  The vertices are a sub-sequence of the ones without
    it.  The final mask share of the result and the final masks of ``mask_folder`` are those of the emit mask.
    normals: every vertex carries nx, ny, nz (``itermvs_fuse_points_normals`` in place of ``itermvs_fuse_points``, 27-byte records,
    the header of ``ply_header(n, normals=True)``): the unit normal of the averaged depth map's surface at the pixel, facing the
    reference camera; ``normal_edge_thres``: relative depth step beyond which a neighbouring pixel is not used for it.  The
    vertices, their order and every other byte are those without it.
    -> {ref_view: (geo, photo, final mask share)} like ``filter_depth``."""
    dev = torch.device(device)
    clock = time.perf_counter
    seconds = {"upload": 0.0, "enqueue": 0.0, "gpu_wait": 0.0, "download_wait": 0.0, "file_write": 0.0, "mask_write": 0.0}
    n_sync = n_chunks = 0
    rec = ops.POINT_NORMAL_RECORD_BYTES if normals else ops.POINT_RECORD_BYTES
    emit = ops.fuse_points_normals if normals else ops.fuse_points
    emit_options = {"edge_thres": normal_edge_thres} if normals else {}
    with torch.cuda.device(dev):
        t0 = clock()
        as_t = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, dt).contiguous()  # noqa: E731
        on_dev = {}
        for ref, srcs in pairs:                                        # every map is uploaded once
            for v in (ref, *srcs):
                if v not in on_dev:
                    on_dev[v] = as_t(depths[v], torch.float32)
        h, w = on_dev[pairs[0][0]].shape if pairs else (1, 1)
        claimed = {v: torch.zeros((h, w), device=dev, dtype=torch.uint8) for v in on_dev} if dedupe else None
        conf = [as_t(confidences[ref], torch.float32) for ref, _ in pairs]
        rgb = [as_t(images[ref], torch.uint8) for ref, _ in pairs]
        for ref, t in zip((p[0] for p in pairs), rgb):
            if tuple(t.shape) != (h, w, 3):
                raise ValueError(f"view {ref}: image is {tuple(t.shape[:2])}, depth map is {(h, w)}")
        f32 = lambda m: np.asarray(m, np.float32)                      # noqa: E731
        mats, cam = [], []
        for ref, srcs in pairs:
            k_ref, e_ref = f32(cams[ref][0]), f32(cams[ref][1])
            mats.append(np.stack([pair_matrices(k_ref, e_ref, f32(cams[v][0]), f32(cams[v][1])) for v in srcs]))
            cam.append(np.concatenate([np.linalg.inv(k_ref).reshape(-1), np.linalg.inv(e_ref)[:3].reshape(-1)]))   # eval.py:291-294
        first_mat = np.cumsum([0] + [len(m) for m in mats])
        mats = torch.from_numpy(np.concatenate(mats)).to(dev) if pairs else None
        cam = torch.from_numpy(np.stack(cam).astype(np.float32)).to(dev) if pairs else None
        groups = group_views(len(pairs), h, w, records_budget, rec)
        capacity = max((b - a) * h * w for a, b in groups) if group_capacity is None and groups else int(group_capacity or 0)
        records = torch.empty(capacity * rec, device=dev, dtype=torch.uint8)
        cursor = torch.zeros(1, device=dev, dtype=torch.int64)
        counts = torch.zeros((max(len(pairs), 1), 4), device=dev, dtype=torch.int64)
        workspace = torch.empty(ops.fuse_points_workspace_bytes(h, w), device=dev, dtype=torch.uint8)
        host = torch.empty((len(pairs) + 1, 4), dtype=torch.int64, pin_memory=True)    # the counts' landing place; last row: cursor
        stream = torch.cuda.current_stream()
        seconds["upload"] = clock() - t0

        stats, spooled, n_vertices = {}, [], 0
        with _remove_on_error(plyfilename), open(plyfilename, "wb") as f:
            for a, b in groups:
                t0 = clock()
                cursor.zero_()
                masks = []
                for i in range(a, b):
                    ref, srcs = pairs[i]
                    maps = (on_dev[ref], conf[i], [on_dev[v] for v in srcs], mats[first_mat[i]:first_mat[i + 1]])
                    thres = (geo_pixel_thres, geo_depth_thres, photo_thres, geo_mask_thres)
                    if dedupe:
                        avg, photo, geo, final, _ = ops.fuse_depth_claim(*maps, claimed[ref], [claimed[v] for v in srcs], *thres)
                    else:
                        avg, photo, geo, final, _ = ops.fuse_depth(*maps, *thres)
                    emit(avg, final, cam[i], rgb[i], records, cursor, counts, i, photo, geo, capacity, workspace, **emit_options)
                    if mask_folder is not None:
                        masks.append((ref, photo, geo, final))
                host[a:b].copy_(counts[a:b], non_blocking=True)
                host[-1, :1].copy_(cursor, non_blocking=True)
                t1 = clock()
                stream.synchronize()                                   # the group's only synchronisation
                n_sync += 1
                t2 = clock()
                seconds["enqueue"] += t1 - t0
                seconds["gpu_wait"] += t2 - t1
                n = int(host[-1, 0])
                if n > capacity:
                    raise RuntimeError(f"fuse_scan: reference views {a}..{b - 1} emit {n} vertices, the records buffer holds "
                                       f"{capacity} (records_budget {records_budget} bytes); nothing was written past it")
                for i in range(a, b):
                    ph, g, fin = (int(c) / float(h * w) for c in host[i, :3])
                    stats[pairs[i][0]] = (g, ph, fin)
                n_vertices += n
                if b == len(pairs):                                    # the total is known: header, earlier groups, then stream
                    t3 = clock()
                    f.write(ply_header(n_vertices, normals))
                    for part in spooled:
                        f.write(part)
                    seconds["file_write"] += clock() - t3
                    n_chunks += _download(records, n * rec, f.write, seconds)
                else:
                    n_chunks += _download(records, n * rec, lambda part: spooled.append(part.copy()), seconds)
                t3 = clock()
                for ref, photo, geo, final in masks:
                    _save_view_masks(mask_folder, ref, photo, geo, final)
                seconds["mask_write"] += clock() - t3
            if not groups:
                f.write(ply_header(0, normals))
    if info is not None:
        info.update(groups=groups, synchronisations=n_sync, downloads=len(groups), download_chunks=n_chunks,
                    vertices=n_vertices, capacity=capacity, seconds=seconds, dedupe=bool(dedupe),
                    normals=bool(normals), record_bytes=rec)
    return stats


def filter_depth(scan_folder: str, out_folder: str, plyfilename: str, geo_pixel_thres: float, geo_depth_thres: float,
                 photo_thres: float, images: Dict[int, np.ndarray] = None, intrinsics_scale: Tuple[float, float] = None,
                 geo_mask_thres: int = 3, device: str = "cuda", img_wh: Tuple[int, int] = None, points: str = "host",
                 save_masks: bool = False, records_budget: int = 2 << 30, info: dict = None,
                 dedupe: bool = False, normals: bool = False, normal_edge_thres: float = 0.01) -> Dict[str, float]:
    """eval.py:215-309: for every reference view of ``pair.txt`` fuse its depth map with its source views' and append the
    surviving pixels to one point cloud.

    Like the reference (eval.py:231-232, 251-252) the ``cams_1`` intrinsics of EVERY view are rescaled by
    ``img_wh / original image size`` and the points are coloured from the resized reference image.  Either
      * ``img_wh`` = (width, height) of the depth maps: ``<scan_folder>/images/{view:08d}.jpg`` is opened for its original
        size (and, for reference views, its pixels); a missing image raises -- the filter refuses to run with a guessed K; or
      * ``images[view]`` = [H,W,3] float RGB in 0..1 at the depth maps' resolution plus ``intrinsics_scale`` =
        (img_w / original_w, img_h / original_h) for callers that hold the images already (default (1, 1)).

    ``points``: where eval.py:287-308 runs.  "host" (default): numpy on the downloaded maps, one synchronisation per reference
    view.  "device": ``fuse_scan`` -- the same files are read, the vertex records are built by ``itermvs_fuse_points`` and the
    host synchronises once per group of reference views (``records_budget`` bytes of records per group; ``info`` as in
    ``fuse_scan``); same header, vertex order and colours, coordinates equal up to the last float64 bit of ``np.matmul``.
    ``save_masks``: also write ``<out_folder>/mask/{view:0>8}_photo.png``, ``_geo.png``, ``_final.png`` (eval.py:266-269).
    ``dedupe``: ``fuse_scan``'s, so it needs ``points="device"``.  ``normals``, ``normal_edge_thres``: ``fuse_scan``'s, with the
    same need."""
    if points not in ("host", "device"):
        raise ValueError(f"filter_depth: points must be 'host' or 'device', got {points!r}")
    if dedupe and points != "device":
        raise ValueError("filter_depth: dedupe=True needs points='device' (the claim maps live on the GPU between the reference "
                         f"views), got points={points!r}")
    if normals and points != "device":
        raise ValueError("filter_depth: normals=True needs points='device' (the normals are computed from the fused depth map on "
                         f"the GPU while the vertices are emitted), got points={points!r}")
    pairs = read_pair_file(os.path.join(scan_folder, "pair.txt"))
    mask_folder = os.path.join(out_folder, "mask") if save_masks else None
    if img_wh is None and images is None and intrinsics_scale is None:
        raise ValueError("filter_depth: pass img_wh (images/ folder is read for the original sizes and colours) or "
                         "images + intrinsics_scale; fusing with unscaled intrinsics would be silently wrong")
    cams, depths, pixels = {}, {}, {}

    def image_path(v):
        base = os.path.join(scan_folder, "images/{:0>8}".format(v))
        for ext in (".jpg", ".png", ".jpeg"):
            if os.path.isfile(base + ext):
                return base + ext
        raise FileNotFoundError(f"{base}.jpg: the filter needs every view's image for the intrinsics scale (eval.py:231-232)")

    def scale_of(v, want_pixels):
        if img_wh is None:
            return intrinsics_scale or (1.0, 1.0)
        px, oh, ow = read_scan_image(image_path(v), img_wh, want_pixels, as_uint8=points == "device")
        if px is not None:
            pixels[v] = px
        return img_wh[0] / ow, img_wh[1] / oh

    def cam(v, want_pixels=False):
        if v not in cams or (want_pixels and img_wh is not None and v not in pixels):
            k, e = read_camera_parameters(os.path.join(scan_folder, "cams_1/{:0>8}_cam.txt".format(v)))
            sx, sy = scale_of(v, want_pixels)
            k = k.copy()
            k[0] *= sx           # python float * float32 row -> float32, like eval.py:231-232
            k[1] *= sy
            cams[v] = (k, e)
        return cams[v]

    def depth(v):
        if v not in depths:
            d = read_pfm(os.path.join(out_folder, "depth_est/{:0>8}.pfm".format(v)))[0]
            depths[v] = torch.from_numpy(np.ascontiguousarray(np.squeeze(d))).to(device)
        return depths[v]

    def confidence(v):
        return np.squeeze(read_pfm(os.path.join(out_folder, "confidence/{:0>8}.pfm".format(v)))[0])

    if points == "device":
        rgb, confs = {}, {}
        for ref_view, src_views in pairs:
            cam(ref_view, want_pixels=True)
            for v in (ref_view, *src_views):
                cam(v)
                depth(v)
            confs[ref_view] = confidence(ref_view)
            h, w = depths[ref_view].shape
            if images is not None:
                rgb[ref_view] = (np.asarray(images[ref_view]) * 255).astype(np.uint8)       # eval.py:296 on the host
            else:
                rgb[ref_view] = pixels.pop(ref_view) if ref_view in pixels else np.full((h, w, 3), 127, np.uint8)
        return fuse_scan(pairs, cams, depths, confs, rgb, plyfilename, geo_pixel_thres, geo_depth_thres, photo_thres,
                         geo_mask_thres, device, records_budget, mask_folder, info=info, dedupe=dedupe, normals=normals,
                         normal_edge_thres=normal_edge_thres)

    vertexs, colors, stats = [], [], {}
    for ref_view, src_views in pairs:
        k_ref, e_ref = cam(ref_view, want_pixels=True)
        conf = confidence(ref_view)
        avg, photo, geo, final, _ = fuse_reference_view(depth(ref_view), conf, k_ref, e_ref, [depth(v) for v in src_views],
                                                        [cam(v)[0] for v in src_views], [cam(v)[1] for v in src_views],
                                                        geo_pixel_thres, geo_depth_thres, photo_thres, geo_mask_thres, device)
        final_np = final.cpu().numpy().astype(bool)
        if save_masks:
            _save_view_masks(mask_folder, ref_view, photo, geo, final)
        stats[ref_view] = (float(geo.float().mean()), float(photo.float().mean()), float(final.float().mean()))
        h, w = final_np.shape
        x, y = np.meshgrid(np.arange(0, w), np.arange(0, h))
        x, y, d = x[final_np], y[final_np], avg.cpu().numpy()[final_np]
        xyz_ref = np.matmul(np.linalg.inv(k_ref), np.vstack((x, y, np.ones_like(x))) * d)          # eval.py:291-292
        xyz_world = np.matmul(np.linalg.inv(e_ref), np.vstack((xyz_ref, np.ones_like(x))))[:3]    # eval.py:293-294
        vertexs.append(xyz_world.transpose((1, 0)))
        if images is not None:
            img = images[ref_view]
        elif ref_view in pixels:
            img = pixels.pop(ref_view)
        else:
            img = np.full((h, w, 3), 0.5, np.float32)
        if img.shape[:2] != (h, w):
            raise ValueError(f"view {ref_view}: image is {img.shape[:2]}, depth map is {(h, w)}")
        colors.append((img[final_np] * 255).astype(np.uint8))
    write_ply(plyfilename, np.concatenate(vertexs, 0).astype(np.float32), np.concatenate(colors, 0))
    return stats
