#!/usr/bin/env python3
"""Simplify a triangle mesh on the GPU by vertex clustering with quadric placement:

    python simplify_mesh.py IN.ply OUT.ply --cell 0.004          # one vertex per occupied cell of side 0.004 (world units)

IN.ply is a binary little-endian mesh as ``eval.py --mesh`` writes it (15-byte coloured vertex records, int32 index triples).  The
vertices are binned into cells of side --cell on a grid whose origin is the per-axis minimum of the finite vertices; every occupied
cell keeps one vertex, placed at the minimiser of the plane quadrics of the cell's triangles (Lindstrom 2000) and clamped to the
cell, with the mean colour; a triangle whose corners fall into fewer than three cells goes, like the later copy of a triangle that
another one repeats with the same orientation.  This is ``eval.py --mesh --mesh_simplify F`` for a mesh that already exists: the same
call, and for --cell = F x the voxel of that run (it prints the number) the same bytes.  --cell has no default."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Vertex-clustering simplification of a PLY triangle mesh (MI355X engine)")
    p.add_argument("src", metavar="IN.ply")
    p.add_argument("dst", metavar="OUT.ply")
    p.add_argument("--cell", type=float, default=None, metavar="C", help="the cell's side in world units (no default)")
    p.add_argument("--device", default="cuda")
    return p


def check_args(args) -> None:
    """no --cell, a value that is not finite and above 0, and OUT.ply == IN.ply are argparse errors (exit status 2)"""
    from itermvs_amd import fusion
    error = build_parser().error
    if args.cell is None:
        error("give --cell C: there is no default cell side")
    problem = fusion.simplify_problem(args.cell)
    if problem:
        error(problem.replace("cell", "--cell", 1))
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
    vertices, kept = fusion.simplify_mesh(torch.from_numpy(records.view(np.uint8).reshape(-1)).to(dev),
                                          torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(-1)).to(dev), args.cell, info=info)
    fusion.write_ply_mesh(args.dst, vertices.cpu().numpy(), kept.cpu().numpy())
    print("{}: {} vertices, {} triangles, {} occupied cells of side {!r}".format(
        args.src, info["vertices_before"], info["faces_before"], info["clusters"], info["cell"]))
    print("kept {} vertices, {} triangles ({} triangles collapsed, {} repeated another)".format(
        info["vertices"], info["faces"], info["degenerate_faces"], info["duplicate_faces"]))
    print("wrote {}".format(args.dst))
    return info


if __name__ == "__main__":
    main()
