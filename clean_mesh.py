#!/usr/bin/env python3
"""Remove the small connected components (floating fragments) of a triangle mesh on the GPU:

    python clean_mesh.py IN.ply OUT.ply --share 0.05             # components below 5 % of the largest component's triangles
    python clean_mesh.py IN.ply OUT.ply --min_faces 500          # components below 500 triangles
    python clean_mesh.py IN.ply OUT.ply --min_faces 500 --share 0.05     # a component must pass both

IN.ply is a binary little-endian mesh as ``eval.py --mesh`` writes it (15-byte coloured vertex records, int32 index triples).  Two
vertices belong to one component when a chain of triangles links them; sharing one vertex index is enough.  A component stays
when it has at least max(1, --min_faces, ceil(--share x the largest component's triangles)) triangles; the kept vertices and
triangles keep their bytes and their order, the indices are renumbered, a vertex that no triangle references goes.  This is
``eval.py --mesh --mesh_min_component N --mesh_component_share F`` for a mesh that already exists: the same two entry points
(itermvs_mesh_components, itermvs_mesh_keep), the same bytes.  At least one of the two thresholds is required; neither has a
default, --share is the one without a scale."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Connected-component removal of a PLY triangle mesh (MI355X engine)")
    p.add_argument("src", metavar="IN.ply")
    p.add_argument("dst", metavar="OUT.ply")
    p.add_argument("--min_faces", type=int, default=None, metavar="N", help="triangles a component needs to stay (no default)")
    p.add_argument("--share", type=float, default=None, metavar="F",
                   help="share of the largest component's triangles a component needs to stay, in [0, 1] (no default)")
    p.add_argument("--device", default="cuda")
    return p


def check_args(args) -> None:
    """neither threshold, a value out of range and OUT.ply == IN.ply are argparse errors (exit status 2)"""
    from itermvs_amd import fusion
    error = build_parser().error
    if args.min_faces is None and args.share is None:
        error("give --min_faces N, --share F or both: there is no default threshold")
    problem = fusion.component_problem(args.min_faces or 0, 0.0 if args.share is None else args.share)
    if problem:
        error(problem.replace("min_component", "--min_faces").replace("component_share", "--share"))
    if os.path.abspath(args.src) == os.path.abspath(args.dst):
        error("OUT.ply must not be IN.ply")


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    check_args(args)
    import numpy as np
    import torch
    from itermvs_amd import data_io, fusion
    xyz, rgb, faces = data_io.read_ply_mesh(args.src)
    if rgb is None:
        raise SystemExit(f"{args.src}: the vertices carry no red, green, blue: not a mesh of eval.py --mesh")
    records = np.empty(len(xyz), fusion.MESH_VERTEX)
    for i, name in enumerate("xyz"):
        records[name] = xyz[:, i]
    for i, name in enumerate(("red", "green", "blue")):
        records[name] = rgb[:, i]
    dev = torch.device(args.device)
    info = {}
    vertices, kept = fusion.keep_mesh_components(torch.from_numpy(records.view(np.uint8).reshape(-1)).to(dev),
                                                 torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(-1)).to(dev),
                                                 args.min_faces or 0, 0.0 if args.share is None else args.share, info=info)
    fusion.write_ply_mesh(args.dst, vertices.cpu().numpy(), kept.cpu().numpy())
    print("{}: {} vertices, {} triangles, {} components, the largest has {} triangles".format(
        args.src, info["vertices_before"], info["faces_before"], info["components"], info["largest"]))
    print("kept the {} components with at least {} triangles: {} vertices, {} triangles".format(
        info["kept_components"], info["min_faces"], info["vertices"], info["faces"]))
    if info["faces_before"] and not info["faces"]:
        print("warning: nothing is left, {} is an empty mesh".format(args.dst))
    print("wrote {}".format(args.dst))
    return info


if __name__ == "__main__":
    main()
