"""PFM reader / writer for depth and confidence maps -- the on-disk format either side of the hot
path (reference: datasets/data_io.py:6-73; written by eval.py:141-151).

Format: ASCII header ``Pf\\n`` (1 channel) or ``PF\\n`` (3 channels), ``<width> <height>\\n``,
``<scale>\\n`` (negative = little-endian), then rows bottom-to-top as raw float32.
"""
from __future__ import annotations

import os
import re
import sys
from typing import Tuple

import numpy as np


def save_pfm(filename: str, image: np.ndarray, scale: float = 1.0) -> None:
    """data_io.py:45-73: float32 H x W (or H x W x 1 / H x W x 3), stored bottom-up."""
    if image.dtype != np.float32:
        raise ValueError("PFM images must be float32")
    if image.ndim == 3 and image.shape[2] == 3:
        magic = b"PF\n"
    elif image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 1):
        magic = b"Pf\n"
    else:
        raise ValueError("PFM image must be H x W, H x W x 1 or H x W x 3")
    little = image.dtype.byteorder == "<" or (image.dtype.byteorder == "=" and sys.byteorder == "little")
    header = magic + f"{image.shape[1]} {image.shape[0]}\n".encode() + ("%f\n" % (-scale if little else scale)).encode()
    os.makedirs(os.path.dirname(os.path.abspath(filename)), exist_ok=True)
    with open(filename, "wb") as f:
        f.write(header)
        np.ascontiguousarray(image[::-1]).tofile(f)


def read_pfm(filename: str) -> Tuple[np.ndarray, float]:
    """data_io.py:6-42 -> (H x W x C float32 array, scale)."""
    with open(filename, "rb") as f:
        magic = f.readline().decode("utf-8").rstrip()
        if magic not in ("PF", "Pf"):
            raise ValueError("not a PFM file")
        channels = 3 if magic == "PF" else 1
        m = re.match(r"^(\d+)\s(\d+)\s$", f.readline().decode("utf-8"))
        if not m:
            raise ValueError("malformed PFM header")
        width, height = int(m.group(1)), int(m.group(2))
        scale = float(f.readline().rstrip())
        endian = "<" if scale < 0 else ">"
        data = np.fromfile(f, endian + "f4")
    return np.flipud(data.reshape(height, width, channels)).copy(), abs(scale)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_xyz(filename: str) -> np.ndarray:
    """vertex x, y, z of a PLY file as float32 [N,3]: ``ascii`` and ``binary_little_endian``, any further scalar vertex
    properties (normals, colours: DTU's ``stl###_total.ply``, this project's 15-byte records) and any elements after the
    vertices (faces).  Big-endian files, list properties inside the vertex element, an element in front of the vertices and a
    short file raise a ValueError naming the file."""
    def bad(why: str) -> ValueError:
        return ValueError(f"{filename}: {why}")

    with open(filename, "rb") as f:
        if f.readline().strip() != b"ply":
            raise bad("not a PLY file")
        fmt, elements, props, current = None, [], [], None
        while True:
            raw = f.readline()
            if not raw:
                raise bad("PLY header without end_header")
            words = raw.decode("ascii", "replace").split()
            if not words or words[0] in ("comment", "obj_info"):
                continue
            if words[0] == "end_header":
                break
            if words[0] == "format" and len(words) >= 2:
                fmt = words[1]
            elif words[0] == "element" and len(words) == 3:
                current = words[1]
                elements.append((current, int(words[2])))
            elif words[0] == "property" and current == "vertex":
                if words[1] == "list":
                    raise bad("list property inside the vertex element")
                if len(words) != 3 or words[1] not in _PLY_TYPES:
                    raise bad(f"unknown vertex property {' '.join(words[1:])!r}")
                props.append((words[2], _PLY_TYPES[words[1]]))
        if fmt not in ("ascii", "binary_little_endian"):
            raise bad(f"format {fmt!r} is not supported (ascii and binary_little_endian are)")
        if not elements or elements[0][0] != "vertex":
            raise bad("the first element must be the vertices")
        n = elements[0][1]
        names = [p[0] for p in props]
        if len(set(names)) != len(names) or any(a not in names for a in "xyz"):
            raise bad(f"the vertex element needs x, y and z once each, has {names}")
        if fmt == "ascii":
            cols = [names.index(a) for a in "xyz"]
            out = np.empty((n, 3), dtype=np.float32)
            for i in range(n):
                words = f.readline().split()
                if len(words) < len(names):
                    raise bad(f"vertex {i} of {n}: the file is short")
                try:
                    out[i] = [float(words[c]) for c in cols]
                except ValueError:
                    raise bad(f"vertex {i}: not a number") from None
            return out
        dtype = np.dtype([(name, "<" + t) for name, t in props])
        data = np.fromfile(f, dtype=dtype, count=n)
        if data.shape[0] != n:
            raise bad(f"{data.shape[0]} of {n} vertices: the file is short")
    return np.stack([data["x"].astype(np.float32), data["y"].astype(np.float32), data["z"].astype(np.float32)], 1)


def read_ply_mesh(filename: str):
    """a binary little-endian triangle mesh as ``fusion.write_ply_mesh`` writes it (``eval.py --mesh``) -> (xyz float32 [N,3], rgb
    uint8 [N,3] or None when the vertices carry no colour, faces int32 [M,3]).  The vertex element comes first and holds scalar
    properties with x, y, z; the face element follows with ONE property, ``list uchar int vertex_indices`` (``uint`` and the
    name ``vertex_index`` are accepted).  Anything else -- ascii, a face that is no triangle, an index outside the vertices, a short
    or overlong file -- raises a ValueError naming the file."""
    def bad(why: str) -> ValueError:
        return ValueError(f"{filename}: {why}")

    with open(filename, "rb") as f:
        if f.readline().strip() != b"ply":
            raise bad("not a PLY file")
        fmt, elements, props, face_props, current = None, [], [], [], None
        while True:
            raw = f.readline()
            if not raw:
                raise bad("PLY header without end_header")
            words = raw.decode("ascii", "replace").split()
            if not words or words[0] in ("comment", "obj_info"):
                continue
            if words[0] == "end_header":
                break
            if words[0] == "format" and len(words) >= 2:
                fmt = words[1]
            elif words[0] == "element" and len(words) == 3:
                current = words[1]
                elements.append((current, int(words[2])))
            elif words[0] == "property" and current == "vertex":
                if len(words) != 3 or words[1] not in _PLY_TYPES:
                    raise bad(f"unsupported vertex property {' '.join(words[1:])!r}")
                props.append((words[2], _PLY_TYPES[words[1]]))
            elif words[0] == "property" and current == "face":
                face_props.append(words[1:])
        if fmt != "binary_little_endian":
            raise bad(f"format {fmt!r} is not supported (binary_little_endian is)")
        if [e[0] for e in elements] != ["vertex", "face"]:
            raise bad(f"expected the elements vertex, face, got {[e[0] for e in elements]}")
        names = [p[0] for p in props]
        if len(set(names)) != len(names) or any(a not in names for a in "xyz"):
            raise bad(f"the vertex element needs x, y and z once each, has {names}")
        if len(face_props) != 1 or face_props[0][:2] != ["list", "uchar"] or len(face_props[0]) != 4 or \
                face_props[0][2] not in ("int", "int32", "uint", "uint32") or face_props[0][3] not in ("vertex_indices", "vertex_index"):
            raise bad(f"the face element needs one property list uchar int vertex_indices, has {face_props}")
        (_, n), (_, m) = elements
        data = np.fromfile(f, dtype=np.dtype([(name, "<" + t) for name, t in props]), count=n)
        if data.shape[0] != n:
            raise bad(f"{data.shape[0]} of {n} vertices: the file is short")
        rows = np.fromfile(f, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]), count=m)
        if rows.shape[0] != m:
            raise bad(f"{rows.shape[0]} of {m} faces: the file is short")
        if f.read(1):
            raise bad("bytes after the last face")
    if m and (rows["n"] != 3).any():
        raise bad("a face that is not a triangle")
    faces = np.ascontiguousarray(rows["v"])
    if m and (faces.min() < 0 or faces.max() >= n):
        raise bad(f"a vertex index outside 0..{n - 1}")
    xyz = np.stack([data[a].astype(np.float32) for a in "xyz"], 1)
    rgb = np.stack([data[a].astype(np.uint8) for a in ("red", "green", "blue")], 1) if all(a in names for a in ("red", "green", "blue")) else None
    return xyz, rgb, faces
