"""Depth-map filtering and fusion after inference (the reference's ``filter_depth``, eval.py:215-309) on the GPU:
one ``itermvs_fuse_depth`` launch per reference view instead of ~40 full-frame numpy passes per (reference, source)
pair.  Host side: the text formats of a scan folder (``pair.txt``, ``cams_1/*_cam.txt``, eval.py:56-65,90-100), PFM
depth / confidence maps (datasets/data_io.py) and the fused point cloud as a binary little-endian PLY with the vertex
layout of eval.py:298-308 (x, y, z float32; red, green, blue uint8)."""
from __future__ import annotations

import contextlib
import dataclasses
import math
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

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


def read_scaled_camera(scan_folder: str, view: int, sx: float, sy: float) -> Tuple[np.ndarray, np.ndarray]:
    """``cams_1/{view:0>8}_cam.txt`` with the intrinsics rescaled to the depth maps' size like eval.py:231-232: a python float
    times a float32 row stays float32.  The files and the memory path of the fusion get byte-identical clouds from this one copy."""
    k, e = read_camera_parameters(os.path.join(scan_folder, "cams_1/{:0>8}_cam.txt".format(view)))
    k = k.copy()
    k[0] *= sx
    k[1] *= sy
    return k, e


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


def dynamic_problem(dyn_pixel_step, dyn_depth_step, dyn_n_min, dyn_n_max) -> Optional[str]:
    """which part of a level rule the entry point would refuse: "steps" (the pixel step as a double and the depth step AS THE
    FLOAT32 IT IS PASSED AS must be finite and above 0: 1e-60 rounds to 0, 1e60 to inf), "levels" (1 <= n_min <= n_max <=
    ITERMVS_MAX_SRC) or None.  The callers word their own messages."""
    with np.errstate(over="ignore"):
        a, b = float(dyn_pixel_step), float(np.float32(dyn_depth_step))
    if not (0 < a < float("inf") and 0 < b < float("inf")):
        return "steps"
    if not 1 <= int(dyn_n_min) <= int(dyn_n_max) <= ops.MAX_SRC:
        return "levels"
    return None


def dynamic_options(consistency: str = "static", dyn_pixel_step: float = ops.DYN_PIXEL_STEP, dyn_depth_step: float = ops.DYN_DEPTH_STEP,
                    dyn_n_min: int = ops.DYN_N_MIN, dyn_n_max: int = ops.DYN_N_MAX) -> Optional[dict]:
    """``consistency`` "static": None (the count against ``geo_mask_thres``); "dynamic": the checked keyword arguments of the
    level rule for ``fuse_view`` (include/itermvs_hip.h: itermvs_fuse_depth_dynamic)"""
    if consistency not in ("static", "dynamic"):
        raise ValueError(f"consistency must be 'static' or 'dynamic', got {consistency!r}")
    if consistency == "static":
        return None
    problem = dynamic_problem(dyn_pixel_step, dyn_depth_step, dyn_n_min, dyn_n_max)
    if problem == "steps":
        raise ValueError(f"dynamic consistency: dyn_pixel_step and dyn_depth_step (as float32) must be finite and above 0, got "
                         f"{dyn_pixel_step}, {dyn_depth_step}")
    if problem == "levels":
        raise ValueError(f"dynamic consistency: the levels must satisfy 1 <= dyn_n_min <= dyn_n_max <= {ops.MAX_SRC}, got "
                         f"{dyn_n_min}..{dyn_n_max}")
    return dict(dyn_pixel_step=float(dyn_pixel_step), dyn_depth_step=float(dyn_depth_step), dyn_n_min=int(dyn_n_min),
                dyn_n_max=int(dyn_n_max))


def consistency_from_args(args) -> dict:
    """the ``--geo_consistency`` / ``--dyn_*`` flags of eval.py -> the keyword arguments ``fuse_scan`` and ``filter_depth`` take"""
    given = lambda name, default: default if getattr(args, name, None) is None else getattr(args, name)      # noqa: E731
    levels = given("dyn_levels", (ops.DYN_N_MIN, ops.DYN_N_MAX))
    return dict(consistency=getattr(args, "geo_consistency", "static"), dyn_pixel_step=given("dyn_pixel_step", ops.DYN_PIXEL_STEP),
                dyn_depth_step=given("dyn_depth_step", ops.DYN_DEPTH_STEP), dyn_n_min=levels[0], dyn_n_max=levels[1])


def fuse_keywords_from_args(args, mesh_path: str) -> dict:
    """the fusion flags of eval.py -> the keyword arguments both drivers pass to ``filter_depth`` / ``fuse_scan``: the four
    thresholds, ``dedupe``, ``normals``, ``normal_edge_thres``, ``mesh`` (written to ``mesh_path``) and the consistency rule"""
    return dict(geo_pixel_thres=args.geo_pixel_thres, geo_depth_thres=args.geo_depth_thres, photo_thres=args.photo_thres,
                geo_mask_thres=args.geo_mask_thres, dedupe=bool(getattr(args, "fuse_dedupe", False)),
                normals=bool(getattr(args, "ply_normals", False)), normal_edge_thres=float(getattr(args, "normal_edge_thres", 0.01)),
                mesh=mesh_options_from_args(args, mesh_path), **consistency_from_args(args))


def print_view_shares(scan: str, stats: Dict[int, Tuple[float, float, float]]) -> None:
    """the line eval.py:270-272 prints per reference view"""
    for v, (g, ph, f) in stats.items():
        print("processing {}, ref-view{:0>2}, geo_mask:{:3f} photo_mask:{:3f} final_mask: {:3f}".format(scan, v, g, ph, f))


def fuse_view(depth_ref, conf_ref, depth_src: Sequence, mats, geo_pixel_thres, geo_depth_thres, photo_thres, geo_mask_thres,
              dyn: Optional[dict] = None, claims: Optional[tuple] = None):
    """one reference view on the GPU through the entry point its options ask for, the only place that chooses: ``dyn`` (what
    ``dynamic_options`` returns) -> ``itermvs_fuse_depth_dynamic``, which takes no ``geo_mask_thres``, with or without ``claims`` =
    (claimed_ref, claimed_src); static with claims -> ``itermvs_fuse_depth_claim``; else ``itermvs_fuse_depth``.  -> that call's tuple"""
    maps, thres = (depth_ref, conf_ref, depth_src, mats), (geo_pixel_thres, geo_depth_thres, photo_thres)
    if dyn is not None:
        return ops.fuse_depth_dynamic(*maps, *(claims or (None, None)), *thres, **dyn)
    if claims is not None:
        return ops.fuse_depth_claim(*maps, *claims, *thres, geo_mask_thres)
    return ops.fuse_depth(*maps, *thres, geo_mask_thres)


def fuse_reference_view(depth_ref, conf_ref, k_ref, e_ref, src_depths: Sequence, src_ks: Sequence, src_es: Sequence,
                        geo_pixel_thres=1.0, geo_depth_thres=0.01, photo_thres=0.3, geo_mask_thres=3, device="cuda",
                        consistency="static", dyn_pixel_step=ops.DYN_PIXEL_STEP, dyn_depth_step=ops.DYN_DEPTH_STEP,
                        dyn_n_min=ops.DYN_N_MIN, dyn_n_max=ops.DYN_N_MAX):
    """eval.py:238-269 for one reference view (numpy or torch inputs) -> torch tensors
    (depth_est_averaged float64, photo_mask, geo_mask, final_mask uint8, geo_mask_sum int32).  ``consistency="dynamic"``: the
    geometric mask is the level rule of ``itermvs_fuse_depth_dynamic`` with the four ``dyn_*`` parameters, ``geo_mask_thres`` is not
    used and the accepting level map (uint8) is returned as a sixth tensor."""
    dev = torch.device(device)
    dyn = dynamic_options(consistency, dyn_pixel_step, dyn_depth_step, dyn_n_min, dyn_n_max)
    as_t = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, torch.float32)
    mats = np.stack([pair_matrices(np.asarray(k_ref), np.asarray(e_ref), np.asarray(k), np.asarray(e))
                     for k, e in zip(src_ks, src_es)])
    return fuse_view(as_t(depth_ref), as_t(conf_ref), [as_t(d) for d in src_depths], torch.from_numpy(mats).to(dev),
                     geo_pixel_thres, geo_depth_thres, photo_thres, geo_mask_thres, dyn)


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


MESH_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
MESH_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])            # property list uchar int vertex_indices: 13 bytes
MESH_KEPT_BYTES_PER_PIXEL = 9                                      # depth_avg float64 + (photo & geo) uint8 per reference view
MESH_INTEGRATE_BATCH = 4                                           # views per itermvs_tsdf_integrate launch (profiles/mesh/README.md)


@dataclasses.dataclass
class MeshOptions:
    """what ``fuse_scan(mesh=...)`` needs.  path: the mesh PLY.  bounds: (x0, y0, z0, x1, y1, z1) of the volume, used as given; None:
    the ``bounds_quantile`` rule of ``mesh_bounds`` on the emitted cloud, widened by the truncation distance.  voxel: the voxel's
    side; None: the longest side of the (unwidened) bounds / ``resolution``.  trunc_voxels: truncation distance in voxels.
    min_count: views a voxel needs to be valid.  budget_bytes: GPU memory the kept views, the volume, the extraction workspace and
    the mesh buffers may take together.  batch_views: views per integrate launch.  The defaults are choices, not measured optima.
    min_component (triangles) and component_share (of the largest component's triangles, in [0, 1]): the connected components of the
    mesh with fewer triangles than ``mesh_min_faces`` makes of the two are left out of the file; both 0: no filter, no kernel.
    simplify_voxels: 0: nothing more; above 0: the mesh of ``path`` is also simplified by ``simplify_mesh`` with cells of that many
    voxels and written to ``simplified_path(path)``; ``path`` itself keeps its bytes."""
    path: str
    bounds: Optional[Sequence[float]] = None
    bounds_quantile: float = 0.01
    voxel: Optional[float] = None
    resolution: int = 256
    trunc_voxels: float = 3.0
    min_count: int = 2
    budget_bytes: int = 16 << 30
    batch_views: int = MESH_INTEGRATE_BATCH
    min_component: int = 0
    component_share: float = 0.0
    # an attribute beside the fields, set by the constructor: dataclasses.asdict, == and the field list describe <path> itself, as
    # before; the second file is an addition to it (dataclasses.replace() must be given the value again: mesh_options does)
    simplify_voxels: dataclasses.InitVar[float] = 0.0

    def __post_init__(self, simplify_voxels):
        self.simplify_voxels = simplify_voxels


def mesh_options(mesh) -> Optional[MeshOptions]:
    """None, a ``MeshOptions`` or a dict of its fields -> a checked ``MeshOptions`` or None"""
    if mesh is None:
        return None
    m = mesh if isinstance(mesh, MeshOptions) else MeshOptions(**dict(mesh))
    finite = lambda x: -float("inf") < float(x) < float("inf")           # noqa: E731
    if m.bounds is not None:
        b = tuple(float(x) for x in m.bounds)
        if len(b) != 6 or not all(finite(x) for x in b) or not all(b[i] < b[i + 3] for i in range(3)):
            raise ValueError(f"mesh: bounds must be six finite numbers x0 y0 z0 x1 y1 z1 with x0 < x1, y0 < y1, z0 < z1, got {m.bounds}")
        m = dataclasses.replace(m, bounds=b, simplify_voxels=m.simplify_voxels)
    if not 0 <= m.bounds_quantile < 0.5:
        raise ValueError(f"mesh: bounds_quantile must be in [0, 0.5), got {m.bounds_quantile}")
    if m.voxel is not None and not (finite(m.voxel) and m.voxel > 0):
        raise ValueError(f"mesh: voxel must be finite and above 0, got {m.voxel}")
    if int(m.resolution) < 2:
        raise ValueError(f"mesh: resolution must be at least 2 voxels, got {m.resolution}")
    if not (finite(m.trunc_voxels) and m.trunc_voxels >= 1):
        raise ValueError(f"mesh: trunc_voxels must be finite and at least 1 (a thinner band misses the voxels next to the surface), "
                         f"got {m.trunc_voxels}")
    if int(m.min_count) < 1 or int(m.batch_views) < 1 or int(m.budget_bytes) < 1:
        raise ValueError(f"mesh: min_count, batch_views and budget_bytes must be at least 1, got {m.min_count}, {m.batch_views}, "
                         f"{m.budget_bytes}")
    problem = component_problem(m.min_component, m.component_share)
    if problem:
        raise ValueError("mesh: " + problem)
    if m.simplify_voxels != 0:
        problem = simplify_problem(m.simplify_voxels)
        if problem:
            raise ValueError("mesh: " + problem.replace("cell", "simplify_voxels", 1))
    return m


def component_problem(min_component, component_share) -> Optional[str]:
    """what is wrong with the two thresholds of the component filter, or None"""
    if isinstance(min_component, bool) or not isinstance(min_component, (int, np.integer)) or not 0 <= int(min_component) <= 0x7fffffff:
        return f"min_component must be a whole number of triangles in [0, 2^31 - 1], got {min_component!r}"
    if isinstance(component_share, bool) or not isinstance(component_share, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(component_share) <= 1.0:
        return f"component_share must be a number in [0, 1], got {component_share!r}"
    return None


def simplify_problem(cell, origin=None) -> Optional[str]:
    """what is wrong with the cell side and the origin of ``simplify_mesh``, or None"""
    number = lambda x: not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating))      # noqa: E731
    if not number(cell) or not 0.0 < float(cell) < float("inf"):
        return f"cell must be a finite number above 0, got {cell!r}"
    if origin is not None:
        try:
            o = tuple(origin)
        except TypeError:
            o = ()
        if len(o) != 3 or not all(number(x) and -float("inf") < float(x) < float("inf") for x in o):
            return f"origin must be three finite numbers, got {origin!r}"
    return None


def simplified_path(path: str) -> str:
    """<scan>_mesh.ply -> <scan>_mesh_simplified.ply"""
    stem, ext = os.path.splitext(path)
    return stem + "_simplified" + ext


def mesh_min_faces(min_component: int, component_share: float, largest: int) -> int:
    """the triangles a component needs to stay, given the ``largest`` component's: a share of exactly k triangles asks for k"""
    return max(1, int(min_component), math.ceil(float(component_share) * int(largest)))


def mesh_options_from_args(args, path: str) -> Optional[MeshOptions]:
    """the ``--mesh*`` flags of eval.py -> ``MeshOptions`` writing ``path``, or None without ``--mesh``"""
    if not getattr(args, "mesh", False):
        return None
    return mesh_options(MeshOptions(path=path, bounds=getattr(args, "mesh_bounds", None),
                                    bounds_quantile=getattr(args, "mesh_bounds_quantile", 0.01), voxel=getattr(args, "mesh_voxel", None),
                                    resolution=getattr(args, "mesh_resolution", 256), trunc_voxels=getattr(args, "mesh_trunc", 3.0),
                                    min_count=getattr(args, "mesh_min_count", 2),
                                    budget_bytes=int(getattr(args, "mesh_budget_gb", 16.0) * (1 << 30)),
                                    min_component=getattr(args, "mesh_min_component", None) or 0,
                                    component_share=getattr(args, "mesh_component_share", None) or 0.0,
                                    simplify_voxels=0.0 if getattr(args, "mesh_simplify", None) is None else args.mesh_simplify))


def mesh_bounds(xyz, quantile: float) -> Tuple[float, ...]:
    """the default volume of a cloud, before widening: per axis the ``quantile`` and ``1 - quantile`` order statistics of the
    finite vertices' coordinates, exact by sort and without interpolation: sorted[k] and sorted[n - 1 - k], k = floor(quantile *
    (n - 1)).  xyz: [n,3] torch tensor (either device) or array.  -> (x0, y0, z0, x1, y1, z1)"""
    t = (xyz if torch.is_tensor(xyz) else torch.from_numpy(np.ascontiguousarray(xyz))).reshape(-1, 3)
    t = t[torch.isfinite(t).all(dim=1)]
    n = t.shape[0]
    if n == 0:
        raise ValueError("mesh_bounds: no finite vertex")
    k = int(math.floor(float(quantile) * (n - 1)))
    s = torch.sort(t, dim=0).values
    lo, hi = s[k].tolist(), s[n - 1 - k].tolist()
    return tuple(float(v) for v in (*lo, *hi))


def mesh_plan(bounds: Sequence[float], voxel: Optional[float] = None, resolution: int = 256, trunc_voxels: float = 3.0,
              widen: bool = True, budget_bytes: int = None, other_bytes: int = 0) -> dict:
    """the volume of a mesh: voxel = ``voxel`` or the longest side of ``bounds`` / ``resolution``; trunc = trunc_voxels * voxel;
    ``widen``: the bounds grow by trunc on every side; dims = ceil(side / voxel) per axis (at least 2, a cell needs two voxels).
    -> {origin, voxel, trunc, dims, state_bytes, workspace_bytes}.  Raises before anything is allocated when state + workspace +
    ``other_bytes`` (what the caller already holds for the mesh) exceed ``budget_bytes``, or the voxel count the 2^32 - 256 of one launch."""
    b = [float(x) for x in bounds]
    sides = [b[i + 3] - b[i] for i in range(3)]
    if not all(s > 0 and s < float("inf") for s in sides):
        raise ValueError(f"mesh_plan: bounds without extent: {tuple(b)}")
    vox = float(voxel) if voxel is not None else max(sides) / int(resolution)
    trunc = float(trunc_voxels) * vox
    origin = [b[i] - (trunc if widen else 0.0) for i in range(3)]
    dims = [max(2, int(math.ceil((sides[i] + (2 * trunc if widen else 0.0)) / vox))) for i in range(3)]
    n = dims[0] * dims[1] * dims[2]
    state_bytes = n * ops.TSDF_VOXEL_BYTES
    workspace_bytes = 16 * ((n + 255) // 256) + 12 * n               # itermvs_tsdf_mesh_workspace_bytes, without the library
    need = state_bytes + workspace_bytes + int(other_bytes)
    hint = "lower --mesh_resolution, raise --mesh_voxel or tighten --mesh_bounds"
    if n > (1 << 32) - 256:
        raise ValueError(f"mesh: a volume of {dims[0]}x{dims[1]}x{dims[2]} voxels is beyond the {(1 << 32) - 256} of one launch; {hint}")
    if budget_bytes is not None and need > budget_bytes:
        raise ValueError(f"mesh: a volume of {dims[0]}x{dims[1]}x{dims[2]} voxels needs {need} bytes on the GPU ({state_bytes} state, "
                         f"{workspace_bytes} extraction workspace, {int(other_bytes)} kept views), the budget is {budget_bytes}; "
                         f"{hint}, or raise --mesh_budget_gb")
    return dict(origin=tuple(origin), voxel=vox, trunc=trunc, dims=tuple(dims), state_bytes=state_bytes,
                workspace_bytes=workspace_bytes, need_bytes=need)


def ply_mesh_header(n_vertices: int, n_faces: int) -> bytes:
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (n_vertices, n_faces)).encode("ascii")


def write_ply_mesh(filename: str, vertices: np.ndarray, faces: np.ndarray) -> None:
    """binary little-endian PLY: ``vertices`` MESH_VERTEX [n] (or their uint8 bytes), ``faces`` int32 [m,3]"""
    vertices = np.ascontiguousarray(vertices).view(np.uint8).reshape(-1, MESH_VERTEX.itemsize)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    rows = np.empty(len(faces), MESH_FACE)
    rows["n"], rows["v"] = 3, faces
    with _remove_on_error(filename), open(filename, "wb") as f:
        f.write(ply_mesh_header(len(vertices), len(faces)))
        f.write(vertices.tobytes())
        f.write(rows.tobytes())


def extract_mesh(state: torch.Tensor, plan: dict, min_count: int, budget_bytes: int = None, used_bytes: int = 0):
    """marching tetrahedra over an integrated volume -> (vertex bytes uint8 [nv*15], faces int32 [nf*3]) on the GPU.  Two runs of
    ``itermvs_tsdf_mesh``: the first with capacities 0 for the totals, the second into buffers of exactly that size; between them the
    buffers are checked against what the budget has left."""
    dev = state.device
    args = (state, plan["dims"], plan["origin"], plan["voxel"], int(min_count))
    totals = torch.zeros(2, device=dev, dtype=torch.int64)
    workspace = torch.empty(ops.tsdf_mesh_workspace_bytes(plan["dims"]), device=dev, dtype=torch.uint8)

    def check(nv, nf, out_bytes):
        if nv > 0x7fffffff:
            raise ValueError(f"mesh: {nv} vertices do not fit the int32 indices of a PLY face; lower --mesh_resolution or raise --mesh_voxel")
        if budget_bytes is not None and used_bytes + out_bytes > budget_bytes:
            raise ValueError(f"mesh: {nv} vertices and {nf} triangles need {out_bytes} bytes on top of {used_bytes}, the budget is "
                             f"{budget_bytes}; lower --mesh_resolution, raise --mesh_voxel or raise --mesh_budget_gb")

    return _count_then_fill(lambda v, f: ops.tsdf_mesh(*args, v, f, totals, workspace), totals, ops.MESH_VERTEX_BYTES, check)


def _count_then_fill(launch, totals: torch.Tensor, vertex_bytes: int, check):
    """the two runs of a kernel that writes a mesh of unknown size: ``launch(vertices, faces)`` with capacities 0 leaves the vertex
    and triangle totals in ``totals`` (int64 [2], on the GPU); they are read, ``check(vertices, triangles, output bytes)`` raises what
    the caller refuses, the buffers are allocated at exactly that size and, unless both are empty, ``launch`` fills them.
    -> (vertex bytes uint8 [nv*vertex_bytes], faces int32 [nf*3])"""
    dev = totals.device
    launch(torch.empty(0, device=dev, dtype=torch.uint8), torch.empty(0, device=dev, dtype=torch.int32))
    nv, nf = (int(t) for t in totals.tolist())
    check(nv, nf, nv * vertex_bytes + nf * ops.MESH_FACE_BYTES)
    vertices = torch.empty(nv * vertex_bytes, device=dev, dtype=torch.uint8)
    faces = torch.empty(nf * 3, device=dev, dtype=torch.int32)
    if nv or nf:
        launch(vertices, faces)
    return vertices, faces


def keep_mesh_components(vertices: torch.Tensor, faces: torch.Tensor, min_component: int = 0, component_share: float = 0.0,
                         budget_bytes: int = None, used_bytes: int = 0, info: dict = None, record_bytes: int = ops.MESH_VERTEX_BYTES):
    """the connected components of a mesh on the GPU (vertex bytes uint8 [nv*record_bytes], faces int32 [nf*3], as ``extract_mesh``
    returns them) with at least ``mesh_min_faces`` triangles -> (vertices, faces) of the same form, in their order, the faces
    renumbered.  ``itermvs_mesh_components``, one read of its three totals, then ``itermvs_mesh_keep`` twice like ``extract_mesh``:
    with capacities 0 for the totals, then into buffers of exactly that size.  The labels, counts, workspace and kept buffers are
    checked against what the budget has left before they are allocated.  ``info`` receives the counts."""
    problem = component_problem(min_component, component_share)
    if problem:
        raise ValueError("mesh: " + problem)
    dev, rec = faces.device, int(record_bytes)
    nv, nf = vertices.numel() // rec, faces.numel() // 3
    label_bytes, count_bytes, workspace_bytes = 4 * nv, 4 * nv, ops.mesh_keep_workspace_bytes(nv, nf)
    hint = "lower --mesh_resolution, raise --mesh_voxel or raise --mesh_budget_gb"
    if budget_bytes is not None and used_bytes + label_bytes + count_bytes + workspace_bytes > budget_bytes:
        raise ValueError(f"mesh: the component filter of {nv} vertices and {nf} triangles needs {label_bytes} bytes of labels, "
                         f"{count_bytes} of counts and {workspace_bytes} of workspace on top of {used_bytes}, the budget is "
                         f"{budget_bytes}; {hint}")
    label, face_count, totals = ops.mesh_components(faces, nv)
    components, largest, valid = (int(t) for t in totals.tolist())
    min_faces = mesh_min_faces(min_component, component_share, largest)
    workspace = torch.empty(max(workspace_bytes, 8), device=dev, dtype=torch.uint8)
    kept = torch.zeros(2, device=dev, dtype=torch.int64)
    args = (vertices, rec, faces, label, face_count, min_faces)

    def check(kv, kf, out_bytes):
        if budget_bytes is not None and used_bytes + label_bytes + count_bytes + workspace_bytes + out_bytes > budget_bytes:
            raise ValueError(f"mesh: the kept {kv} vertices and {kf} triangles need {out_bytes} bytes on top of {used_bytes} and the "
                             f"component filter's {label_bytes + count_bytes + workspace_bytes} (labels, counts, workspace), the budget "
                             f"is {budget_bytes}; {hint}")

    out_vertices, out_faces = _count_then_fill(lambda v, f: ops.mesh_keep(*args, v, f, kept, workspace), kept, rec, check)
    if info is not None:
        kept_components = int((face_count >= min_faces).sum()) if nv else 0
        info.update(components=components, largest=largest, min_faces=min_faces, kept_components=kept_components,
                    valid_faces=valid, vertices_before=nv, faces_before=nf, vertices=out_vertices.numel() // rec,
                    faces=out_faces.numel() // 3, component_bytes=label_bytes + count_bytes + workspace_bytes)
    return out_vertices, out_faces


SIMPLIFY_SORT_BYTES_PER_VERTEX = 64        # coordinates, keys, sorted keys, order, heads, prefix sums, cluster numbers (twice)
SIMPLIFY_SORT_BYTES_PER_FACE = 148         # the 3 pairs (values, sorted values, order, faces), the triple keys and their two sorts


def simplify_grid(xyz: torch.Tensor, cell: float, origin=None) -> ops.CloudGrid:
    """the grid of ``simplify_mesh`` over float32 [n,3] coordinates: ``origin`` or, for None, the per-axis minimum of the finite
    vertices (exact: a float32 as a double); cells up to the finite vertices' maximum.  One synchronisation (the extent comes to the
    host, as in ``cloud_grid.grid_for``); more than 2^21 cells on an axis raise"""
    from . import cloud_grid
    finite = torch.isfinite(xyz).all(1)
    inf = float("inf")
    lo = torch.where(finite[:, None], xyz, torch.full_like(xyz, inf)).min(0).values.double()
    hi = torch.where(finite[:, None], xyz, torch.full_like(xyz, -inf)).max(0).values.double()
    lo, hi = torch.stack([lo, hi]).tolist()
    if not all(-inf < v < inf for v in lo):                           # no finite vertex
        return ops.CloudGrid(tuple(float(o) for o in origin) if origin is not None else (0.0, 0.0, 0.0), (1, 1, 1), float(cell))
    o = [float(v) for v in (lo if origin is None else origin)]
    dims = [max(1, int(math.floor((hi[a] - o[a]) / float(cell))) + 1) for a in range(3)]
    if max(dims) > cloud_grid.MAX_CELL_DIM:
        raise ValueError(f"simplify_mesh: the mesh spans {dims} cells of side {cell}; at most {cloud_grid.MAX_CELL_DIM} per axis fit "
                         "the cell key (choose a larger cell)")
    return ops.CloudGrid(tuple(o), tuple(dims), float(cell))


def simplify_clusters(vertices: torch.Tensor, flat: torch.Tensor, rec: int, xyz: torch.Tensor, grid: ops.CloudGrid):
    """everything of ``simplify_mesh`` before the compaction, nothing read back: the three stable sorts and the two launches
    between them -> (reps, cluster, key_hi_sorted, key_lo_sorted, order: the arguments of ``ops.mesh_simplify_emit``; counts: a
    function that reads clusters, valid and alive faces back)"""
    nv, dev = xyz.shape[0], flat.device
    none = torch.iinfo(torch.int64).max
    keys_sorted, perm = torch.sort(ops.cloud_cell_keys(xyz, grid), stable=True)
    cluster_sorted = torch.where(keys_sorted != none, torch.cumsum(ops.cloud_voxel_heads(keys_sorted), 0) - 1, -1).to(torch.int32)
    cluster = torch.empty(nv, device=dev, dtype=torch.int32)
    cluster[perm] = cluster_sorted
    pair, key_hi, key_lo = ops.mesh_simplify_corners(flat, cluster)
    pair_sorted, pair_order = torch.sort(pair, stable=True)                    # face-major pairs, by cluster
    pair_face = torch.div(pair_order, 3, rounding_mode="floor").to(torch.int32)
    by_lo = torch.sort(key_lo, stable=True).indices                            # the canonical triples: by c2, then by (c0, c1)
    key_hi_sorted, by_hi = torch.sort(key_hi[by_lo], stable=True)
    order = by_lo[by_hi]
    key_lo_sorted, order = key_lo[order], order.to(torch.int32)
    reps = ops.mesh_simplify_clusters(vertices, rec, flat, keys_sorted, perm, cluster_sorted, pair_sorted, pair_face, grid)

    def counts():
        nf = key_hi.numel()
        return (int(cluster_sorted.max()) + 1 if nv else 0, int((pair[0::3] != 0x7fffffff).sum()) if nf else 0,
                int((key_hi != none).sum()) if nf else 0)

    return reps, cluster, key_hi_sorted, key_lo_sorted, order, counts


def simplify_mesh(vertices: torch.Tensor, faces: torch.Tensor, cell: float, origin=None, info: dict = None, budget_bytes: int = None,
                  used_bytes: int = 0, record_bytes: int = ops.MESH_VERTEX_BYTES, dims=None):
    """vertex clustering with quadric placement on the GPU (include/itermvs_hip.h: rules 1..6): vertex bytes uint8
    [nv*record_bytes] and faces int32 [nf*3], as ``extract_mesh`` returns them -> (vertices, faces) of the same form, one vertex per
    occupied cell of side ``cell`` that a surviving triangle references.  ``origin``: the grid's corner; None: the per-axis minimum
    of the valid vertices.  ``dims``: the grid's cells per axis, with ``origin``; None: up to the vertices' maximum.
    The three stable sorts (vertices by cell key, the 3 nf (cluster, face) pairs by cluster, the canonical triples) are torch.sort; keys
    and run heads are ``itermvs_cloud_cell_keys`` / ``itermvs_cloud_voxel_heads``; the rest is ``itermvs_mesh_simplify_*``, the last of
    them twice like ``extract_mesh``.  One synchronisation for the extent and one for the totals.  The buffers are checked against
    what the budget has left before they are allocated.  ``info`` receives the counts, ``cell`` and ``origin``."""
    problem = simplify_problem(cell, origin)
    if problem:
        raise ValueError("simplify_mesh: " + problem)
    if dims is not None and origin is None:
        raise ValueError("simplify_mesh: dims needs an origin")
    dev, rec = faces.device, int(record_bytes)
    if not 12 <= rec <= 64 or vertices.numel() % rec or faces.numel() % 3:
        raise ValueError(f"simplify_mesh: {vertices.numel()} vertex bytes are no records of {rec} bytes (12..64), or {faces.numel()} "
                         "indices no triples")
    nv, nf = vertices.numel() // rec, faces.numel() // 3
    if nf > ops.MESH_SIMPLIFY_MAX_FACES:
        raise ValueError(f"simplify_mesh: {nf} triangles are beyond the {ops.MESH_SIMPLIFY_MAX_FACES} of one launch")
    sort_bytes = SIMPLIFY_SORT_BYTES_PER_VERTEX * nv + SIMPLIFY_SORT_BYTES_PER_FACE * nf
    reps_bytes, workspace_bytes = rec * nv, ops.mesh_simplify_emit_workspace_bytes(nv, nf)
    own_bytes = sort_bytes + reps_bytes + workspace_bytes
    hint = "lower --mesh_resolution, raise --mesh_voxel or raise --mesh_budget_gb"
    if budget_bytes is not None and used_bytes + own_bytes > budget_bytes:
        raise ValueError(f"mesh: the simplifier of {nv} vertices and {nf} triangles needs {sort_bytes} bytes of keys and sort orders, "
                         f"{reps_bytes} of representatives and {workspace_bytes} of workspace on top of {used_bytes}, the budget is "
                         f"{budget_bytes}; {hint}")
    flat = faces.reshape(-1)
    xyz = vertices.view(nv, rec)[:, :12].contiguous().view(torch.float32) if nv else torch.empty((0, 3), device=dev, dtype=torch.float32)
    if nv:
        grid = simplify_grid(xyz, cell, origin) if dims is None else ops.CloudGrid(tuple(float(o) for o in origin),
                                                                                   tuple(int(d) for d in dims), float(cell))
    else:
        grid = ops.CloudGrid(tuple(float(o) for o in origin) if origin is not None else (0.0, 0.0, 0.0), (1, 1, 1), float(cell))
    reps, cluster, key_hi_sorted, key_lo_sorted, order, counts = simplify_clusters(vertices, flat, rec, xyz, grid)
    workspace = torch.empty(max(workspace_bytes, 8), device=dev, dtype=torch.uint8)
    totals = torch.zeros(2, device=dev, dtype=torch.int64)

    def check(kv, kf, out_bytes):
        if budget_bytes is not None and used_bytes + own_bytes + out_bytes > budget_bytes:
            raise ValueError(f"mesh: the simplified {kv} vertices and {kf} triangles need {out_bytes} bytes on top of {used_bytes} and "
                             f"the simplifier's {own_bytes} (keys and sort orders, representatives, workspace), the budget is "
                             f"{budget_bytes}; {hint}")

    out_vertices, out_faces = _count_then_fill(
        lambda v, f: ops.mesh_simplify_emit(reps, rec, flat, cluster, key_hi_sorted, key_lo_sorted, order, v, f, totals, workspace),
        totals, rec, check)
    if info is not None:
        clusters, valid_faces, alive = counts()
        info.update(vertices_before=nv, faces_before=nf, vertices=out_vertices.numel() // rec, faces=out_faces.numel() // 3,
                    clusters=clusters, valid_faces=valid_faces, degenerate_faces=valid_faces - alive,
                    duplicate_faces=alive - out_faces.numel() // 3, cell=float(cell), origin=tuple(grid.origin), dims=tuple(grid.dims),
                    simplify_bytes=own_bytes)
    return out_vertices, out_faces


def write_scan_mesh(mesh: MeshOptions, bounds: Sequence[float], depth: torch.Tensor, mask: torch.Tensor, cams: torch.Tensor,
                    rgb: torch.Tensor, info: dict = None) -> None:
    """the kept views (depth float64 [V,H,W], mask uint8 [V,H,W], cams float32 [V,21] = K | E[:3], rgb uint8 [V,H,W,3], on the GPU, in
    pair.txt order) -> ``mesh.path``: the volume of ``mesh_plan``, ``itermvs_tsdf_integrate`` in batches of ``mesh.batch_views``,
    ``extract_mesh``, ``keep_mesh_components`` when ``mesh.min_component`` or ``mesh.component_share`` is set, one download (of the
    kept mesh alone)"""
    v, h, w = depth.shape
    kept = v * h * w * MESH_KEPT_BYTES_PER_PIXEL
    plan = mesh_plan(bounds, mesh.voxel, mesh.resolution, mesh.trunc_voxels, widen=mesh.bounds is None,
                     budget_bytes=mesh.budget_bytes, other_bytes=kept)
    state = ops.tsdf_volume(plan["dims"], depth.device)
    for a in range(0, v, int(mesh.batch_views)):
        b = min(a + int(mesh.batch_views), v)
        ops.tsdf_integrate(state, plan["dims"], plan["origin"], plan["voxel"], plan["trunc"], depth[a:b], mask[a:b], cams[a:b], rgb[a:b])
    vertices, faces = extract_mesh(state, plan, mesh.min_count, mesh.budget_bytes, plan["need_bytes"])
    kept_info = {}
    if mesh.min_component or mesh.component_share:
        had = vertices.numel() + faces.numel() * 4
        vertices, faces = keep_mesh_components(vertices, faces, mesh.min_component, mesh.component_share, mesh.budget_bytes,
                                               plan["need_bytes"] + had, kept_info)
        if had and not faces.numel():
            kept_info.update(warning=f"mesh: no component has {kept_info['min_faces']} triangles (the largest has "
                                     f"{kept_info['largest']}): {mesh.path} is an empty mesh")
    write_ply_mesh(mesh.path, vertices.cpu().numpy(), faces.cpu().numpy())
    if info is not None:
        info.update(plan, bounds=tuple(bounds), vertices=vertices.numel() // ops.MESH_VERTEX_BYTES, faces=faces.numel() // 3,
                    batches=(v + int(mesh.batch_views) - 1) // int(mesh.batch_views))
        info.update(kept_info)
    if mesh.simplify_voxels:
        simplified = write_simplified_mesh(mesh.path, vertices, faces, float(mesh.simplify_voxels) * plan["voxel"], mesh.budget_bytes,
                                           plan["need_bytes"] + vertices.numel() + faces.numel() * 4)
        if info is not None:
            info.update(simplified=simplified)


def write_simplified_mesh(path: str, vertices: torch.Tensor, faces: torch.Tensor, cell: float, budget_bytes: int = None,
                          used_bytes: int = 0) -> dict:
    """the mesh that ``path`` holds (on the GPU) -> ``simplified_path(path)`` by ``simplify_mesh`` with the default origin, and one
    printed line with both triangle counts and the cell in world units as ``repr``: ``simplify_mesh.py --cell`` with that number
    repeats the file.  -> the simplifier's ``info``"""
    info = {}
    out_vertices, out_faces = simplify_mesh(vertices, faces, cell, info=info, budget_bytes=budget_bytes, used_bytes=used_bytes)
    write_ply_mesh(simplified_path(path), out_vertices.cpu().numpy(), out_faces.cpu().numpy())
    print("simplified {}: {} -> {} triangles, {} -> {} vertices, cell {!r}, wrote {}".format(
        path, info["faces_before"], info["faces"], info["vertices_before"], info["vertices"], info["cell"], simplified_path(path)))
    return info


class _DeviceScan:
    """a scan on the GPU, built once per ``fuse_scan``: depth[view] float32 [H,W] (every map is uploaded once), conf[i] and rgb[i] of
    the i-th reference view, the pair blocks of all views in ``mats`` (view i's are mats[first_mat[i]:first_mat[i + 1]]), the ``cam``
    rows inv(K) | inv(E)[:3] of eval.py:291-294 and, with ``dedupe``, one zeroed uint8 claim map per view"""

    def __init__(self, pairs, cams, depths, confidences, images, dev, dedupe: bool):
        as_t = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, dt).contiguous()  # noqa: E731
        f32 = lambda m: np.asarray(m, np.float32)                      # noqa: E731
        self.pairs, self.depth = pairs, {}
        for ref, srcs in pairs:
            for v in (ref, *srcs):
                if v not in self.depth:
                    self.depth[v] = as_t(depths[v], torch.float32)
        self.h, self.w = h, w = self.depth[pairs[0][0]].shape if pairs else (1, 1)
        self.claimed = {v: torch.zeros((h, w), device=dev, dtype=torch.uint8) for v in self.depth} if dedupe else None
        self.conf = [as_t(confidences[ref], torch.float32) for ref, _ in pairs]
        self.rgb = [as_t(images[ref], torch.uint8) for ref, _ in pairs]
        for (ref, _), t in zip(pairs, self.rgb):
            if tuple(t.shape) != (h, w, 3):
                raise ValueError(f"view {ref}: image is {tuple(t.shape[:2])}, depth map is {(h, w)}")
        mats, cam = [], []
        for ref, srcs in pairs:
            k_ref, e_ref = f32(cams[ref][0]), f32(cams[ref][1])
            mats.append(np.stack([pair_matrices(k_ref, e_ref, f32(cams[v][0]), f32(cams[v][1])) for v in srcs]))
            cam.append(np.concatenate([np.linalg.inv(k_ref).reshape(-1), np.linalg.inv(e_ref)[:3].reshape(-1)]))
        self.first_mat = np.cumsum([0] + [len(m) for m in mats])
        self.mats = torch.from_numpy(np.concatenate(mats)).to(dev) if pairs else None
        self.cam = torch.from_numpy(np.stack(cam).astype(np.float32)).to(dev) if pairs else None

    def inputs(self, i: int) -> tuple:
        """(depth_ref, conf_ref, [depth_src], mats) of the i-th reference view"""
        ref, srcs = self.pairs[i]
        return self.depth[ref], self.conf[i], [self.depth[v] for v in srcs], self.mats[self.first_mat[i]:self.first_mat[i + 1]]

    def claims(self, i: int) -> Optional[tuple]:
        """(claimed_ref, [claimed_src]) of the i-th reference view, None without ``dedupe``"""
        ref, srcs = self.pairs[i]
        return (self.claimed[ref], [self.claimed[v] for v in srcs]) if self.claimed is not None else None


class _RecordBuffer:
    """where the views of a group leave their vertices and counts, allocated once per scan: ``records`` for ``capacity`` vertices (the
    largest group's worst case unless ``group_capacity`` is given), the ``cursor``, the per-view ``counts``, the emit kernels'
    ``workspace`` and the pinned ``host`` rows the counts land in (last row: the cursor)"""

    def __init__(self, scan: _DeviceScan, rec: int, groups, group_capacity: Optional[int], records_budget: int, dev):
        n, h, w = len(scan.pairs), scan.h, scan.w
        self.scan, self.records_budget = scan, records_budget
        self.capacity = max((b - a) * h * w for a, b in groups) if group_capacity is None and groups else int(group_capacity or 0)
        self.records = torch.empty(self.capacity * rec, device=dev, dtype=torch.uint8)
        self.cursor = torch.zeros(1, device=dev, dtype=torch.int64)
        self.counts = torch.zeros((max(n, 1), 4), device=dev, dtype=torch.int64)
        self.workspace = torch.empty(ops.fuse_points_workspace_bytes(h, w), device=dev, dtype=torch.uint8)
        self.host = torch.empty((n + 1, 4), dtype=torch.int64, pin_memory=True)

    def enqueue_landing(self, a: int, b: int) -> None:
        self.host[a:b].copy_(self.counts[a:b], non_blocking=True)
        self.host[-1, :1].copy_(self.cursor, non_blocking=True)

    def landed(self, a: int, b: int, stats: dict) -> int:
        """after the group's synchronisation: stats[ref_view] = (geo, photo, final mask share) of views a..b-1 -> vertices emitted"""
        n, pixels = int(self.host[-1, 0]), float(self.scan.h * self.scan.w)
        if n > self.capacity:
            raise RuntimeError(f"fuse_scan: reference views {a}..{b - 1} emit {n} vertices, the records buffer holds "
                               f"{self.capacity} (records_budget {self.records_budget} bytes); nothing was written past it")
        for i in range(a, b):
            ph, g, fin = (int(c) / pixels for c in self.host[i, :3])
            stats[self.scan.pairs[i][0]] = (g, ph, fin)
        return n


class _PlyAppender:
    """the header-last rule of the cloud's file ``f``: the vertex total is known only with the last group, so the groups before it
    are spooled as host copies; the last one writes the header, the spooled parts and streams its own records through ``download``"""

    def __init__(self, f, normals: bool, seconds: Dict[str, float], download):
        self.f, self.normals, self.seconds, self.download = f, normals, seconds, download
        self.spooled, self.vertices, self.chunks, self.headed = [], 0, 0, False

    def append(self, records, n: int, rec: int, last: bool) -> None:
        self.vertices += n
        if not last:
            self.chunks += self.download(records, n * rec, lambda part: self.spooled.append(part.copy()), self.seconds)
            return
        t0 = time.perf_counter()
        self.f.write(ply_header(self.vertices, self.normals))
        for part in self.spooled:
            self.f.write(part)
        self.seconds["file_write"] += time.perf_counter() - t0
        self.headed = True
        self.chunks += self.download(records, n * rec, self.f.write, self.seconds)


@contextlib.contextmanager
def _open_cloud(filename: str, normals: bool, seconds: Dict[str, float], download=_download):
    """-> the ``_PlyAppender`` of ``filename``; a scan without groups gets the empty header, a raise inside removes the file"""
    with _remove_on_error(filename), open(filename, "wb") as f:
        ply = _PlyAppender(f, normals, seconds, download)
        yield ply
        if not ply.headed:
            f.write(ply_header(0, normals))


class _MeshKeeper:
    """what ``fuse_scan(mesh=...)`` holds on the GPU while the cloud is assembled: every reference view's ``depth_avg`` and
    ``photo & geo``, the colours as one tensor (``scan.rgb`` becomes its views: the emit kernels read the same memory) and, for the
    default bounds, the emitted coordinates of every group.  The kept views are checked against the budget before they are allocated."""

    def __init__(self, mesh: MeshOptions, scan: _DeviceScan, dev):
        self.mesh, self.pairs, self.cloud_xyz = mesh, scan.pairs, []
        n, h, w = len(scan.pairs), scan.h, scan.w
        if not n:
            return
        kept_bytes = n * h * w * MESH_KEPT_BYTES_PER_PIXEL
        if kept_bytes > mesh.budget_bytes:
            raise ValueError(f"mesh: keeping {n} fused {w}x{h} views on the GPU takes {kept_bytes} bytes, the budget is "
                             f"{mesh.budget_bytes} (mesh budget_bytes)")
        self.depth = torch.empty((n, h, w), device=dev, dtype=torch.float64)
        self.mask = torch.empty((n, h, w), device=dev, dtype=torch.uint8)
        self.rgb = torch.stack(scan.rgb)
        scan.rgb = list(self.rgb)

    def keep_view(self, i: int, avg, photo, geo) -> None:
        self.depth[i].copy_(avg)
        self.mask[i].copy_((photo != 0) & (geo != 0))

    def note_group(self, records, n: int, rec: int) -> None:
        if self.mesh.bounds is None and n:
            self.cloud_xyz.append(records[:n * rec].view(n, rec)[:, :12].contiguous().view(torch.float32))

    def finish(self, cams, dev) -> dict:
        """after the last group: the bounds (given, or ``mesh_bounds`` of the emitted cloud) and ``write_scan_mesh``; a scan without
        reference views gets the empty mesh file.  -> the mesh's ``info``"""
        info = {}
        if not self.pairs:
            write_ply_mesh(self.mesh.path, np.zeros(0, MESH_VERTEX), np.zeros((0, 3), np.int32))
            if self.mesh.simplify_voxels:
                write_ply_mesh(simplified_path(self.mesh.path), np.zeros(0, MESH_VERTEX), np.zeros((0, 3), np.int32))
            return info
        bounds = self.mesh.bounds
        if bounds is None:
            if not self.cloud_xyz:
                raise ValueError("mesh: the cloud is empty, there is nothing to take the default bounds from (give bounds)")
            bounds = mesh_bounds(torch.cat(self.cloud_xyz), self.mesh.bounds_quantile)
        self.cloud_xyz = None
        f32 = lambda m: np.asarray(m, np.float32)                      # noqa: E731
        kcam = np.stack([np.concatenate([f32(cams[ref][0]).reshape(-1), f32(cams[ref][1])[:3].reshape(-1)])
                         for ref, _ in self.pairs]).astype(np.float32)
        write_scan_mesh(self.mesh, bounds, self.depth, self.mask, torch.from_numpy(kcam).to(dev), self.rgb, info=info)
        return info


def fuse_scan(pairs: Sequence[Tuple[int, Sequence[int]]], cams, depths, confidences, images, plyfilename: str,
              geo_pixel_thres: float, geo_depth_thres: float, photo_thres: float, geo_mask_thres: int = 3, device: str = "cuda",
              records_budget: int = 2 << 30, mask_folder: str = None, group_capacity: int = None,
              info: dict = None, dedupe: bool = False, normals: bool = False,
              normal_edge_thres: float = 0.01, mesh=None, consistency: str = "static", dyn_pixel_step: float = ops.DYN_PIXEL_STEP,
              dyn_depth_step: float = ops.DYN_DEPTH_STEP, dyn_n_min: int = ops.DYN_N_MIN,
              dyn_n_max: int = ops.DYN_N_MAX) -> Dict[int, Tuple[float, float, float]]:
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
    mesh: ``MeshOptions`` (or a dict of its fields; None: off) -- also write a triangle mesh of the scan (``write_scan_mesh``): every
    reference view's ``depth_avg`` and ``photo & geo`` stay on the GPU while the cloud is assembled (9 bytes per pixel and view, part
    of the mesh's budget), the emitted vertices' coordinates are kept for the default bounds, and after the last group the views are
    integrated into a volume in ``pairs`` order and marching tetrahedra writes ``mesh.path``.  The cloud, the masks and the
    returned shares are those without it.
    consistency: "static" (default): a pixel's geometric mask is ``count >= geo_mask_thres``.  "dynamic": the level rule of
    ``itermvs_fuse_depth_dynamic`` with ``dyn_pixel_step``, ``dyn_depth_step`` and the levels ``dyn_n_min..dyn_n_max`` takes its
    place in one launch of that entry point per reference view, ``geo_mask_thres`` is not used; the cloud, ``dedupe``, ``normals``,
    the mesh's kept mask, the masks of ``mask_folder`` and the returned shares all follow the dynamic ``geo``.
    -> {ref_view: (geo, photo, final mask share)} like ``filter_depth``."""
    dev = torch.device(device)
    mesh = mesh_options(mesh)
    dyn = dynamic_options(consistency, dyn_pixel_step, dyn_depth_step, dyn_n_min, dyn_n_max)
    thres = (geo_pixel_thres, geo_depth_thres, photo_thres, geo_mask_thres)
    rec = ops.POINT_NORMAL_RECORD_BYTES if normals else ops.POINT_RECORD_BYTES
    emit = ops.fuse_points_normals if normals else ops.fuse_points
    emit_options = {"edge_thres": normal_edge_thres} if normals else {}
    clock = time.perf_counter
    seconds = {"upload": 0.0, "enqueue": 0.0, "gpu_wait": 0.0, "download_wait": 0.0, "file_write": 0.0, "mask_write": 0.0}
    stats, n_sync, mesh_info = {}, 0, None
    with torch.cuda.device(dev):
        t0 = clock()
        scan = _DeviceScan(pairs, cams, depths, confidences, images, dev, dedupe)
        keeper = _MeshKeeper(mesh, scan, dev) if mesh is not None else None
        groups = group_views(len(pairs), scan.h, scan.w, records_budget, rec)
        out = _RecordBuffer(scan, rec, groups, group_capacity, records_budget, dev)
        stream = torch.cuda.current_stream()
        seconds["upload"] = clock() - t0
        with _open_cloud(plyfilename, normals, seconds) as ply:
            for a, b in groups:
                t0 = clock()
                out.cursor.zero_()
                masks = []
                for i in range(a, b):                                  # per view: the fuse launch, the emit launch, the mesh copies
                    avg, photo, geo, final = fuse_view(*scan.inputs(i), *thres, dyn, scan.claims(i))[:4]
                    emit(avg, final, scan.cam[i], scan.rgb[i], out.records, out.cursor, out.counts, i, photo, geo, out.capacity,
                         out.workspace, **emit_options)
                    if mask_folder is not None:
                        masks.append((pairs[i][0], photo, geo, final))
                    if keeper is not None:
                        keeper.keep_view(i, avg, photo, geo)
                out.enqueue_landing(a, b)
                t1 = clock()
                stream.synchronize()                                   # the group's only synchronisation
                n_sync += 1
                t2 = clock()
                seconds["enqueue"] += t1 - t0
                seconds["gpu_wait"] += t2 - t1
                n = out.landed(a, b, stats)
                if keeper is not None:
                    keeper.note_group(out.records, n, rec)
                ply.append(out.records, n, rec, last=b == len(pairs))
                t3 = clock()
                for ref, photo, geo, final in masks:
                    _save_view_masks(mask_folder, ref, photo, geo, final)
                seconds["mask_write"] += clock() - t3
        if keeper is not None:
            mesh_info = keeper.finish(cams, dev)
    if info is not None:
        if mesh is not None:
            info.update(mesh=mesh_info)
        info.update(groups=groups, synchronisations=n_sync, downloads=len(groups), download_chunks=ply.chunks,
                    vertices=ply.vertices, capacity=out.capacity, seconds=seconds, dedupe=bool(dedupe),
                    normals=bool(normals), record_bytes=rec, consistency=consistency)
    return stats


def filter_depth(scan_folder: str, out_folder: str, plyfilename: str, geo_pixel_thres: float, geo_depth_thres: float,
                 photo_thres: float, images: Dict[int, np.ndarray] = None, intrinsics_scale: Tuple[float, float] = None,
                 geo_mask_thres: int = 3, device: str = "cuda", img_wh: Tuple[int, int] = None, points: str = "host",
                 save_masks: bool = False, records_budget: int = 2 << 30, info: dict = None,
                 dedupe: bool = False, normals: bool = False, normal_edge_thres: float = 0.01, mesh=None,
                 consistency: str = "static", dyn_pixel_step: float = ops.DYN_PIXEL_STEP, dyn_depth_step: float = ops.DYN_DEPTH_STEP,
                 dyn_n_min: int = ops.DYN_N_MIN, dyn_n_max: int = ops.DYN_N_MAX) -> Dict[str, float]:
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
    same need; ``mesh``: ``fuse_scan``'s, with the same need.  ``consistency`` and the four ``dyn_*`` parameters: ``fuse_scan``'s,
    with either value of ``points``."""
    if points not in ("host", "device"):
        raise ValueError(f"filter_depth: points must be 'host' or 'device', got {points!r}")
    rule = dict(consistency=consistency, dyn_pixel_step=dyn_pixel_step, dyn_depth_step=dyn_depth_step, dyn_n_min=dyn_n_min,
                dyn_n_max=dyn_n_max)
    dynamic_options(**rule)
    for asked, reason in ((dedupe, "dedupe=True needs points='device' (the claim maps live on the GPU between the reference views)"),
                          (normals, "normals=True needs points='device' (the normals are computed from the fused depth map on the GPU "
                                    "while the vertices are emitted)"),
                          (mesh is not None, "mesh needs points='device' (the volume is integrated from the fused depth maps that stay "
                                             "on the GPU)")):
        if asked and points != "device":
            raise ValueError(f"filter_depth: {reason}, got points={points!r}")
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
            cams[v] = read_scaled_camera(scan_folder, v, *scale_of(v, want_pixels))
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
                         normal_edge_thres=normal_edge_thres, mesh=mesh, **rule)

    vertexs, colors, stats = [], [], {}
    for ref_view, src_views in pairs:
        k_ref, e_ref = cam(ref_view, want_pixels=True)
        conf = confidence(ref_view)
        avg, photo, geo, final = fuse_reference_view(depth(ref_view), conf, k_ref, e_ref, [depth(v) for v in src_views],
                                                     [cam(v)[0] for v in src_views], [cam(v)[1] for v in src_views],
                                                     geo_pixel_thres, geo_depth_thres, photo_thres, geo_mask_thres, device, **rule)[:4]
        if save_masks:
            _save_view_masks(mask_folder, ref_view, photo, geo, final)
        stats[ref_view] = (float(geo.float().mean()), float(photo.float().mean()), float(final.float().mean()))
        img = images[ref_view] if images is not None else pixels.pop(ref_view, None)
        xyz, rgb = _host_points(ref_view, avg, final, k_ref, e_ref, img)
        vertexs.append(xyz)
        colors.append(rgb)
    write_ply(plyfilename, np.concatenate(vertexs, 0).astype(np.float32), np.concatenate(colors, 0))
    return stats


def _host_points(ref_view: int, avg, final, k_ref, e_ref, img) -> Tuple[np.ndarray, np.ndarray]:
    """eval.py:287-296 for one reference view with numpy on the downloaded maps: the surviving pixels -> (world coordinates [n,3]
    float64, colours [n,3] uint8); ``img``: float RGB [H,W,3] in 0..1, None: mid grey"""
    final_np = final.cpu().numpy().astype(bool)
    h, w = final_np.shape
    x, y = np.meshgrid(np.arange(0, w), np.arange(0, h))
    x, y, d = x[final_np], y[final_np], avg.cpu().numpy()[final_np]
    xyz_ref = np.matmul(np.linalg.inv(k_ref), np.vstack((x, y, np.ones_like(x))) * d)          # eval.py:291-292
    xyz_world = np.matmul(np.linalg.inv(e_ref), np.vstack((xyz_ref, np.ones_like(x))))[:3]    # eval.py:293-294
    if img is None:
        img = np.full((h, w, 3), 0.5, np.float32)
    if img.shape[:2] != (h, w):
        raise ValueError(f"view {ref_view}: image is {img.shape[:2]}, depth map is {(h, w)}")
    return xyz_world.transpose((1, 0)), (img[final_np] * 255).astype(np.uint8)
