"""COLMAP sparse model -> scan folder (``cams_1/``, ``images/``, ``pair.txt``): the reference's ``colmap_input.py`` with its two
loops on the GPU.

The model files are read from COLMAP's published layout (``src/colmap/scene/reconstruction_io.cc``; little endian):

* ``cameras.bin``  uint64 n, then per camera int32 id, int32 model id, uint64 width, uint64 height, float64 params[model];
* ``images.bin``   uint64 n, then per image int32 id, float64 qvec[4] (w x y z), float64 tvec[3], int32 camera id, the name as a
  NUL-terminated string, uint64 m, m x (float64 x, float64 y, int64 point3D id or -1);
* ``points3D.bin`` uint64 n, then per point uint64 id, float64 xyz[3], uint8 rgb[3], float64 error, uint64 track length L,
  L x (int32 image id, int32 point2D index);
* the ``.txt`` forms hold the same fields space separated, ``#`` comment lines, two lines per image.

Both forms are accepted (the reference's ``__main__`` reads ``.bin`` only); ``read_model`` takes ``.bin`` when all three exist.
**Image index = position in the images file**, not the COLMAP image id (colmap_input.py:276-277, 310).

What the device computes (``itermvs_view_scores``, ``itermvs_depth_ranges``; include/itermvs_hip.h) is colmap_input.py:319-364;
the host keeps file parsing, the 3x3 / 4x4 matrices of V images, ``np.argsort(score[i])[::-1]`` (that very call: the order among
equal scores is numpy's, as in the reference) and the text forms of the three outputs.

Two behaviours of the reference are deliberately NOT reproduced:

* an image without a valid observation makes it raise ``IndexError`` (colmap_input.py:330); here ``ValueError`` names the image;
* a cosine that rounds above 1 makes ``np.arccos`` return NaN there, which poisons the pair's score; the kernel clamps the cosine
  to [-1, 1].
"""
from __future__ import annotations

import argparse
import os
import shutil
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

# model id -> (name, number of parameters); COLMAP src/colmap/sensor/models.h
CAMERA_MODELS: Dict[int, Tuple[str, int]] = {
    0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
    5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5),
    10: ("THIN_PRISM_FISHEYE", 12)}
CAMERA_MODEL_NAMES = {name: (mid, n) for mid, (name, n) in CAMERA_MODELS.items()}
# models whose parameter list starts f, cx, cy; every other one starts fx, fy, cx, cy.  Distortion is ignored (colmap_input.py:279-305)
SINGLE_FOCAL = {"SIMPLE_PINHOLE", "SIMPLE_RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL", "RADIAL_FISHEYE"}

OBSERVATION = np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")])


@dataclass
class Camera:
    id: int
    model: str
    width: int
    height: int
    params: np.ndarray            # float64


@dataclass
class Image:
    id: int
    qvec: np.ndarray              # float64 [4], w x y z
    tvec: np.ndarray              # float64 [3]
    camera_id: int
    name: str
    point3d_ids: np.ndarray       # int64 [m], -1 = no 3-D point, in file order
    xys: Optional[np.ndarray] = None     # float64 [m,2]; kept so a model can be written back


@dataclass
class Model:
    cameras: Dict[int, Camera]
    images: List[Image]
    point_ids: np.ndarray         # int64 [P], in file order
    xyz: np.ndarray               # float64 [P,3]


class _Bytes:
    """bounds-checked cursor over a file's bytes: running off the end is a ValueError naming the file"""

    def __init__(self, path: str):
        self.path = path
        with open(path, "rb") as f:
            self.buf = f.read()
        self.pos = 0

    def take(self, fmt: str):
        n = struct.calcsize(fmt)
        if self.pos + n > len(self.buf):
            raise ValueError(f"{self.path}: truncated (needs {n} bytes at offset {self.pos}, file has {len(self.buf)})")
        out = struct.unpack_from(fmt, self.buf, self.pos)
        self.pos += n
        return out

    def array(self, dtype, count: int) -> np.ndarray:
        n = np.dtype(dtype).itemsize * count
        if self.pos + n > len(self.buf):
            raise ValueError(f"{self.path}: truncated (needs {n} bytes at offset {self.pos}, file has {len(self.buf)})")
        out = np.frombuffer(self.buf, dtype=dtype, count=count, offset=self.pos)
        self.pos += n
        return out

    def cstring(self) -> str:
        end = self.buf.find(b"\x00", self.pos)
        if end < 0:
            raise ValueError(f"{self.path}: truncated (unterminated name at offset {self.pos})")
        out = self.buf[self.pos:end].decode("utf-8")
        self.pos = end + 1
        return out


def read_cameras_binary(path: str) -> Dict[int, Camera]:
    b = _Bytes(path)
    cams: Dict[int, Camera] = {}
    for _ in range(b.take("<Q")[0]):
        cid, mid, w, h = b.take("<iiQQ")
        if mid not in CAMERA_MODELS:
            raise ValueError(f"{path}: camera {cid} has unknown camera model id {mid}")
        name, n = CAMERA_MODELS[mid]
        cams[cid] = Camera(cid, name, w, h, b.array("<f8", n).copy())
    return cams


def read_images_binary(path: str) -> List[Image]:
    b = _Bytes(path)
    images: List[Image] = []
    for _ in range(b.take("<Q")[0]):
        head = b.take("<idddddddi")
        name = b.cstring()
        obs = b.array(OBSERVATION, b.take("<Q")[0])
        images.append(Image(head[0], np.array(head[1:5]), np.array(head[5:8]), head[8], name, obs["id"].astype(np.int64),
                            np.stack([obs["x"], obs["y"]], 1)))
    return images


def read_points3d_binary(path: str) -> Tuple[np.ndarray, np.ndarray]:
    b = _Bytes(path)
    n = b.take("<Q")[0]
    ids, xyz = np.empty(n, np.int64), np.empty((n, 3), np.float64)
    for k in range(n):
        pid, x, y, z, _, _, _, _, track = b.take("<QdddBBBdQ")
        ids[k], xyz[k] = pid, (x, y, z)
        if b.pos + 8 * track > len(b.buf):
            raise ValueError(f"{path}: truncated (track of point {pid} runs past the end of the file)")
        b.pos += 8 * track
    return ids, xyz


def _text_lines(path: str):
    with open(path, "r") as f:
        for line in f:
            yield line.strip()


def read_cameras_text(path: str) -> Dict[int, Camera]:
    cams: Dict[int, Camera] = {}
    for line in _text_lines(path):
        if not line or line[0] == "#":
            continue
        el = line.split()
        if len(el) < 4:
            raise ValueError(f"{path}: truncated camera line {line!r}")
        if el[1] not in CAMERA_MODEL_NAMES:
            raise ValueError(f"{path}: camera {el[0]} has unknown camera model {el[1]}")
        params = np.array([float(x) for x in el[4:]], np.float64)
        if len(params) != CAMERA_MODEL_NAMES[el[1]][1]:
            raise ValueError(f"{path}: truncated: camera {el[0]} ({el[1]}) has {len(params)} parameters")
        cams[int(el[0])] = Camera(int(el[0]), el[1], int(el[2]), int(el[3]), params)
    return cams


def read_images_text(path: str) -> List[Image]:
    images: List[Image] = []
    lines = _text_lines(path)
    for line in lines:
        if not line or line[0] == "#":
            continue
        el = line.split()
        if len(el) < 10:
            raise ValueError(f"{path}: truncated image line {line!r}")
        obs = next(lines, None)                         # the observation line may be empty, but it is there
        if obs is None:
            raise ValueError(f"{path}: truncated (image {el[0]} has no observation line)")
        obs = obs.split()
        if len(obs) % 3:
            raise ValueError(f"{path}: truncated observation line of image {el[0]}")
        images.append(Image(int(el[0]), np.array([float(x) for x in el[1:5]]), np.array([float(x) for x in el[5:8]]), int(el[8]),
                            el[9], np.array([int(x) for x in obs[2::3]], np.int64),
                            np.array([float(x) for x in obs]).reshape(-1, 3)[:, :2].copy()))
    return images


def read_points3d_text(path: str) -> Tuple[np.ndarray, np.ndarray]:
    ids, xyz = [], []
    for line in _text_lines(path):
        if not line or line[0] == "#":
            continue
        el = line.split()
        if len(el) < 8:
            raise ValueError(f"{path}: truncated point line {line!r}")
        ids.append(int(el[0]))
        xyz.append([float(x) for x in el[1:4]])
    return np.array(ids, np.int64), np.array(xyz, np.float64).reshape(-1, 3)


def read_model(path: str, ext: Optional[str] = None) -> Model:
    """the three files of ``path`` (``<input>/sparse``); ``ext`` None: ``.bin`` when all three exist, else ``.txt``"""
    names = ("cameras", "images", "points3D")
    if ext is None:
        for cand in (".bin", ".txt"):
            if all(os.path.isfile(os.path.join(path, n + cand)) for n in names):
                ext = cand
                break
        else:
            raise ValueError(f"{path}: neither cameras/images/points3D.bin nor .txt found")
    files = [os.path.join(path, n + ext) for n in names]
    if ext == ".bin":
        cams, images, (ids, xyz) = read_cameras_binary(files[0]), read_images_binary(files[1]), read_points3d_binary(files[2])
    elif ext == ".txt":
        cams, images, (ids, xyz) = read_cameras_text(files[0]), read_images_text(files[1]), read_points3d_text(files[2])
    else:
        raise ValueError(f"unknown model format {ext!r}")
    return Model(cams, images, ids, xyz)


def write_model(path: str, model: Model, ext: str = ".bin") -> None:
    """the inverse of :func:`read_model` (synthetic models of the tests and of tools/colmap_bench.py).  Colours are 0, errors 0
    and tracks empty: nothing reads them.  ``.txt`` prints floats with ``repr`` so they read back to the same bits."""
    os.makedirs(path, exist_ok=True)
    cams, images = model.cameras, model.images
    xys = [im.xys if im.xys is not None else np.zeros((len(im.point3d_ids), 2)) for im in images]
    if ext == ".bin":
        with open(os.path.join(path, "cameras.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(cams)))
            for c in cams.values():
                f.write(struct.pack("<iiQQ", c.id, CAMERA_MODEL_NAMES[c.model][0], c.width, c.height))
                f.write(np.asarray(c.params, "<f8").tobytes())
        with open(os.path.join(path, "images.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(images)))
            for im, xy in zip(images, xys):
                f.write(struct.pack("<idddddddi", im.id, *[float(x) for x in im.qvec], *[float(x) for x in im.tvec], im.camera_id))
                f.write(im.name.encode("utf-8") + b"\x00")
                obs = np.empty(len(im.point3d_ids), OBSERVATION)
                obs["x"], obs["y"], obs["id"] = xy[:, 0], xy[:, 1], im.point3d_ids
                f.write(struct.pack("<Q", len(obs)))
                f.write(obs.tobytes())
        rec = np.zeros(len(model.point_ids), np.dtype([("id", "<u8"), ("xyz", "<f8", 3), ("rgb", "u1", 3), ("err", "<f8"), ("n", "<u8")]))
        rec["id"], rec["xyz"] = model.point_ids, model.xyz
        with open(os.path.join(path, "points3D.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(rec)))
            f.write(rec.tobytes())
    elif ext == ".txt":
        with open(os.path.join(path, "cameras.txt"), "w") as f:
            f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
            for c in cams.values():
                f.write(" ".join([str(c.id), c.model, str(c.width), str(c.height)] + [repr(float(x)) for x in c.params]) + "\n")
        with open(os.path.join(path, "images.txt"), "w") as f:
            f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                    "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
            for im, xy in zip(images, xys):
                f.write(" ".join([str(im.id)] + [repr(float(x)) for x in im.qvec] + [repr(float(x)) for x in im.tvec]
                                 + [str(im.camera_id), im.name]) + "\n")
                f.write(" ".join(f"{float(x)!r} {float(y)!r} {int(p)}" for (x, y), p in zip(xy, im.point3d_ids)) + "\n")
        with open(os.path.join(path, "points3D.txt"), "w") as f:
            f.write("# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[]\n")
            for pid, p in zip(model.point_ids, model.xyz):
                f.write(" ".join([str(int(pid))] + [repr(float(x)) for x in p] + ["0", "0", "0", "0.0"]) + "\n")
    else:
        raise ValueError(f"unknown model format {ext!r}")


def quaternion_to_rotation_matrix(qvec) -> np.ndarray:
    """colmap_input.py:235-245, on Python floats in the same operation order"""
    q = [float(x) for x in qvec]
    return np.array([
        [1 - 2 * q[2] ** 2 - 2 * q[3] ** 2, 2 * q[1] * q[2] - 2 * q[0] * q[3], 2 * q[3] * q[1] + 2 * q[0] * q[2]],
        [2 * q[1] * q[2] + 2 * q[0] * q[3], 1 - 2 * q[1] ** 2 - 2 * q[3] ** 2, 2 * q[2] * q[3] - 2 * q[0] * q[1]],
        [2 * q[3] * q[1] - 2 * q[0] * q[2], 2 * q[2] * q[3] + 2 * q[0] * q[1], 1 - 2 * q[1] ** 2 - 2 * q[2] ** 2]])


def rotation_matrix_to_quaternion(r) -> np.ndarray:
    """w x y z of a rotation matrix (the branch on the largest diagonal term): what a model WRITER needs; the inverse of
    :func:`quaternion_to_rotation_matrix` up to rounding"""
    r = np.asarray(r, np.float64)
    t = np.trace(r)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = [0.25 * s, (r[2, 1] - r[1, 2]) / s, (r[0, 2] - r[2, 0]) / s, (r[1, 0] - r[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(r)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + r[i, i] - r[j, j] - r[k, k]) * 2
        q = [0.0] * 4
        q[0] = (r[k, j] - r[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (r[j, i] + r[i, j]) / s
        q[1 + k] = (r[k, i] + r[i, k]) / s
    return np.array(q)


def intrinsic_matrix(cam: Camera) -> np.ndarray:
    """fx, fy, cx, cy (or f) of the model's parameter list; distortion ignored (colmap_input.py:293-305)"""
    if cam.model not in CAMERA_MODEL_NAMES:
        raise ValueError(f"camera {cam.id}: unknown camera model {cam.model}")
    p = [float(x) for x in cam.params]
    fx, fy, cx, cy = (p[0], p[0], p[1], p[2]) if cam.model in SINGLE_FOCAL else p[:4]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])


def extrinsic_matrices(images: List[Image]) -> np.ndarray:
    """colmap_input.py:309-315 -> float64 [V,4,4]"""
    out = np.zeros((len(images), 4, 4))
    for i, im in enumerate(images):
        out[i, :3, :3] = quaternion_to_rotation_matrix(im.qvec)
        out[i, :3, 3] = im.tvec
        out[i, 3, 3] = 1
    return out


def camera_centres(extrinsic: np.ndarray) -> np.ndarray:
    """-R^T t per image with the reference's very expression (colmap_input.py:340) -> float64 [V,3]"""
    return np.stack([-np.matmul(e[:3, :3].transpose(), e[:3, 3:4])[:, 0] for e in extrinsic])


def observation_csr(model: Model) -> Tuple[np.ndarray, np.ndarray]:
    """the images' point-id lists as CSR over DENSE point indices (position in ``model.point_ids``) -> (offsets int64 [V+1],
    point int32 [total]); -1 stays -1, file order and repeats are kept.  An id that points3D does not hold is a ValueError (the
    reference fails with a KeyError at its first use)."""
    lens = np.array([len(im.point3d_ids) for im in model.images], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate([im.point3d_ids for im in model.images]) if len(model.images) else np.zeros(0, np.int64)
    if len(model.point_ids) >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 points")
    order = np.argsort(model.point_ids, kind="stable")
    sorted_ids = model.point_ids[order]
    valid = ids != -1
    pos = np.searchsorted(sorted_ids, ids[valid])
    ok = pos < len(sorted_ids)
    ok[ok] = sorted_ids[pos[ok]] == ids[valid][ok]
    if not ok.all():
        bad = int(ids[valid][~ok][0])
        raise ValueError(f"an image observes point3D id {bad}, which points3D does not hold")
    point = np.full(len(ids), -1, np.int32)
    point[valid] = order[pos].astype(np.int32)
    return offsets, point


def device_scores_and_ranges(model: Model, extrinsic: np.ndarray, theta0: float, sigma1: float, sigma2: float, device="cuda"):
    """one upload, the two kernels, one download -> (score float64 [V,V], ranges float64 [V,2]) as numpy arrays"""
    import torch
    from . import ops
    offsets, point = observation_csr(model)
    dev = torch.device(device)
    off_host = torch.from_numpy(offsets)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    off, pt, xyz = up(offsets), up(point), up(model.xyz)
    centre, row2 = up(camera_centres(extrinsic)), up(extrinsic[:, 2, :])
    score = ops.view_scores(off_host, pt, xyz, centre, theta0, sigma1, sigma2, offsets_dev=off)
    ranges = ops.depth_ranges(off_host, pt, xyz, row2, offsets_dev=off)
    v = len(model.images)
    both = torch.cat([score.reshape(-1), ranges.reshape(-1)]).cpu().numpy()          # the one download (and synchronisation)
    return both[:v * v].reshape(v, v).copy(), both[v * v:].reshape(v, 2).copy()


def select_views(score: np.ndarray, num_src_images: int = -1) -> List[List[Tuple[int, float]]]:
    """colmap_input.py:366-372: ALL images by default, image i itself and zero-score images included"""
    n = len(score) if num_src_images < 0 else num_src_images
    return [[(k, score[i, k]) for k in np.argsort(score[i])[::-1][:n]] for i in range(len(score))]


def cam_text(extrinsic: np.ndarray, intrinsic: np.ndarray, depth_min: float, depth_max: float) -> str:
    """colmap_input.py:379-390: ``str`` of each float64 entry followed by a space"""
    out = ["extrinsic\n"]
    for j in range(4):
        out += [str(extrinsic[j, k]) + " " for k in range(4)] + ["\n"]
    out.append("\nintrinsic\n")
    for j in range(3):
        out += [str(intrinsic[j, k]) + " " for k in range(3)] + ["\n"]
    out.append("\n%f %f \n" % (depth_min, depth_max))
    return "".join(out)


def pair_text(view_sel: List[List[Tuple[int, float]]]) -> str:
    """colmap_input.py:392-398"""
    out = ["%d\n" % len(view_sel)]
    for i, row in enumerate(view_sel):
        out.append("%d\n%d " % (i, len(row)))
        out += ["%d %f " % (k, s) for k, s in row]
        out.append("\n")
    return "".join(out)


def write_outputs(output_folder: str, model: Model, extrinsic: np.ndarray, score: np.ndarray, ranges: np.ndarray,
                  num_src_images: int = -1) -> None:
    """``cams_1/%08d_cam.txt`` and ``pair.txt`` in the reference's text forms"""
    for i, im in enumerate(model.images):
        if not np.isfinite(ranges[i]).all():
            raise ValueError(f"image {i} ({im.name}) has no observation of a 3-D point: no depth range can be given")
        if im.camera_id not in model.cameras:
            raise ValueError(f"image {i} ({im.name}) refers to camera {im.camera_id}, which cameras does not hold")
    intrinsic = {cid: intrinsic_matrix(c) for cid, c in model.cameras.items()}
    cam_dir = os.path.join(output_folder, "cams_1")
    os.makedirs(cam_dir, exist_ok=True)
    for i, im in enumerate(model.images):
        with open(os.path.join(cam_dir, "%08d_cam.txt" % i), "w") as f:
            f.write(cam_text(extrinsic[i], intrinsic[im.camera_id], ranges[i, 0], ranges[i, 1]))
    with open(os.path.join(output_folder, "pair.txt"), "w") as f:
        f.write(pair_text(select_views(score, num_src_images)))


def copy_image(src: str, dst: str, convert_format: bool = False) -> None:
    if convert_format:
        from PIL import Image as PILImage
        with PILImage.open(src) as img:
            img.convert("RGB").save(dst, format="JPEG", quality=95)
    elif os.path.abspath(src) != os.path.abspath(dst):
        shutil.copyfile(src, dst)


def copy_images(image_dir: str, renamed_dir: str, images: List[Image], convert_format: bool = False) -> None:
    """colmap_input.py:400-406: ``images/<name>`` -> ``images/%08d.jpg``; ``convert_format`` re-encodes as JPEG (Pillow)"""
    os.makedirs(renamed_dir, exist_ok=True)
    for i, im in enumerate(images):
        copy_image(os.path.join(image_dir, im.name), os.path.join(renamed_dir, "%08d.jpg" % i), convert_format)


MAX_WORKERS = 16


def undistort_images(image_dir: str, renamed_dir: str, model: Model, out_cameras: Dict[int, Camera], convert_format: bool = False,
                     device="cuda", num_workers: int = 4, info: Optional[dict] = None) -> None:
    """``images/<name>`` -> ``images/%08d.jpg`` as the pinhole cameras ``out_cameras`` (camera id -> undistort.undistorted_camera)
    see them: decoded in a thread pool, uploaded as uint8, resampled by ``itermvs_undistort_rgb8``, downloaded and written as JPEG
    of quality 95 in the same pool.  Images of a camera that ``out_cameras`` returns unchanged (no distortion) are copied as
    :func:`copy_images` does.  ``info`` receives the seconds spent decoding, on the device (upload to download) and encoding,
    the first and the last summed over the pool's threads."""
    import time
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    from itertools import islice
    import torch
    from PIL import Image as PILImage
    from . import ops
    os.makedirs(renamed_dir, exist_ok=True)
    workers = max(1, min(int(num_workers), MAX_WORKERS))
    dev = torch.device(device)
    spent = {"decode": 0.0, "device": 0.0, "encode": 0.0}

    def decode(i: int) -> np.ndarray:
        t0 = time.perf_counter()
        im = model.images[i]
        with PILImage.open(os.path.join(image_dir, im.name)) as img:
            raw = np.array(img.convert("RGB"))
        cam = model.cameras[im.camera_id]
        if raw.shape[:2] != (cam.height, cam.width):
            raise ValueError(f"image {i} ({im.name}) is {raw.shape[1]} x {raw.shape[0]}, its camera {cam.id} is {cam.width} x {cam.height}")
        spent["decode"] += time.perf_counter() - t0          # (float adds under the interpreter lock: a statistic, not a ledger)
        return raw

    def encode(i: int, rgb: np.ndarray) -> None:
        t0 = time.perf_counter()
        PILImage.fromarray(rgb).save(os.path.join(renamed_dir, "%08d.jpg" % i), format="JPEG", quality=95)
        spent["encode"] += time.perf_counter() - t0

    warped = [i for i, im in enumerate(model.images) if out_cameras[im.camera_id] is not model.cameras[im.camera_id]]
    for i, im in enumerate(model.images):
        if out_cameras[im.camera_id] is model.cameras[im.camera_id]:
            copy_image(os.path.join(image_dir, im.name), os.path.join(renamed_dir, "%08d.jpg" % i), convert_format)
    with ThreadPoolExecutor(workers) as pool:
        decoded, written, ahead = deque(), [], iter(warped)

        def decode_more(n: int) -> None:                     # at most 2 x workers decoded images wait for the device
            for j in islice(ahead, n):
                decoded.append((j, pool.submit(decode, j)))

        decode_more(2 * workers)
        while decoded:
            i, job = decoded.popleft()
            raw = job.result()
            decode_more(1)
            t0 = time.perf_counter()
            cam, out = model.cameras[model.images[i].camera_id], out_cameras[model.images[i].camera_id]
            rgb = ops.undistort_rgb8(torch.from_numpy(raw).to(dev), cam.model, cam.params, out.params, (out.height, out.width))
            rgb = rgb.cpu().numpy()                           # the download synchronises
            spent["device"] += time.perf_counter() - t0
            written.append(pool.submit(encode, i, rgb))
        for job in written:
            job.result()
    if info is not None:
        info.update(undistort_decode_s=spent["decode"], undistort_device_s=spent["device"], undistort_encode_s=spent["encode"],
                    undistort_images=len(warped))


def convert(input_folder: str, output_folder: Optional[str] = None, num_src_images: int = -1, theta0: float = 5, sigma1: float = 1,
            sigma2: float = 10, convert_format: bool = False, device="cuda", info: Optional[dict] = None, undistort: bool = False,
            blank_pixels: float = 0.0, min_scale: float = 0.2, max_scale: float = 2.0, num_workers: int = 4) -> None:
    """``<input>/sparse`` + ``<input>/images`` -> ``<output>/cams_1``, ``<output>/images``, ``<output>/pair.txt``
    (``output_folder`` None or empty: the input folder, like the reference).  ``info`` receives the stages' wall times.
    ``undistort``: every camera with lens distortion is replaced by the pinhole camera of ``undistort.undistorted_camera``
    (``blank_pixels``, ``min_scale``, ``max_scale``: its options) in the cam files, and its images are resampled to it on the GPU
    (:func:`undistort_images`); ``pair.txt`` and the depth ranges do not depend on the images and stay as they are."""
    import time
    if not output_folder:
        output_folder = input_folder
    if input_folder is None or not os.path.isdir(input_folder):
        raise ValueError("Invalid input folder")
    if not os.path.isdir(output_folder):
        raise ValueError("Invalid output folder")
    t0 = time.perf_counter()
    model = read_model(os.path.join(input_folder, "sparse"))
    if not model.images:
        raise ValueError(f"{input_folder}: the model holds no image")
    t1 = time.perf_counter()
    extrinsic = extrinsic_matrices(model.images)
    score, ranges = device_scores_and_ranges(model, extrinsic, theta0, sigma1, sigma2, device)
    t2 = time.perf_counter()
    t3 = t2
    if undistort:
        from .undistort import undistorted_camera
        out_cameras = {cid: undistorted_camera(c, blank_pixels, min_scale, max_scale) for cid, c in model.cameras.items()}
        write_outputs(output_folder, Model(out_cameras, model.images, model.point_ids, model.xyz), extrinsic, score, ranges,
                      num_src_images)
        t3 = time.perf_counter()
        undistort_images(os.path.join(input_folder, "images"), os.path.join(output_folder, "images"), model, out_cameras,
                         convert_format, device, num_workers, info)
    else:
        write_outputs(output_folder, model, extrinsic, score, ranges, num_src_images)
        copy_images(os.path.join(input_folder, "images"), os.path.join(output_folder, "images"), model.images, convert_format)
    t4 = time.perf_counter()
    if info is not None:
        if undistort:
            info.update(read_s=t1 - t0, device_s=t2 - t1, write_s=t3 - t2, undistort_s=t4 - t3)
        else:
            info.update(read_s=t1 - t0, device_s=t2 - t1, write_s=t4 - t2)
        info.update(images=len(model.images), points=len(model.point_ids))


def build_parser() -> argparse.ArgumentParser:
    """the reference's flags (colmap_input.py:249-258) plus ``--device``"""
    p = argparse.ArgumentParser(description="Convert colmap results into input for IterMVS")
    p.add_argument("--input_folder", type=str, help="Project input dir.")
    p.add_argument("--output_folder", type=str, default="", help="Project output dir.")
    p.add_argument("--num_src_images", type=int, default=-1, help="Related images")
    p.add_argument("--theta0", type=float, default=5)
    p.add_argument("--sigma1", type=float, default=1)
    p.add_argument("--sigma2", type=float, default=10)
    p.add_argument("--convert_format", action="store_true", default=False, help="If set, convert image to jpg format.")
    p.add_argument("--device", type=str, default="cuda", help="device of the score / depth-range kernels")
    p.add_argument("--undistort", action="store_true", default=False,
                   help="resample the images of cameras with lens distortion to pinhole cameras on the GPU and write those cameras")
    p.add_argument("--blank_pixels", type=float, default=0.0, help="--undistort: 0 crops to pixels the source covers, 1 keeps all of it")
    p.add_argument("--min_scale", type=float, default=0.2, help="--undistort: lower bound of the per-axis change of the image size")
    p.add_argument("--max_scale", type=float, default=2.0, help="--undistort: upper bound of the per-axis change of the image size")
    p.add_argument("--num_workers", type=int, default=4, help="--undistort: threads that decode and encode images (at most 16)")
    return p


def main(argv=None) -> None:
    a = build_parser().parse_args(argv)
    convert(a.input_folder, a.output_folder, a.num_src_images, a.theta0, a.sigma1, a.sigma2, a.convert_format, a.device,
            undistort=a.undistort, blank_pixels=a.blank_pixels, min_scale=a.min_scale, max_scale=a.max_scale,
            num_workers=a.num_workers)
