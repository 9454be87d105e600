#!/usr/bin/env python3
"""Remove the outliers of a fused point cloud on the GPU (itermvs_amd.cloud_filter):

    python clean_cloud.py IN.ply OUT.ply                                   # statistical, k 20, std_ratio 2.0
    python clean_cloud.py IN.ply OUT.ply --method radius --radius 0.01 --min_neighbours 4

IN.ply is a binary little-endian PLY as ``eval.py --filter`` writes it (15-byte vertex records, 27 bytes with ``--ply_normals``,
or any scalar vertex properties).  OUT.ply holds the kept vertex records byte for byte and in their original order; only the
vertex count of the header changes.

statistical (Open3D's remove_statistical_outlier): a vertex is removed when the mean distance to its ``--k`` nearest neighbours
exceeds the cloud's mean of that distance by more than ``--std_ratio`` standard deviations, or when fewer than k other vertices
lie within ``--max_dist`` (such a vertex is isolated and takes no part in the mean).  radius (PCL's RadiusOutlierRemoval): a vertex
is removed when fewer than ``--min_neighbours`` other vertices lie within ``--radius``.  The defaults 20, 2.0 and 0.02 x the
diagonal of the 1 % .. 99 % quantile box are choices, not measured optima."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OPTIONS = ("k", "std_ratio", "max_dist", "radius", "min_neighbours")
OWNER = {"k": "statistical", "std_ratio": "statistical", "max_dist": "statistical", "radius": "radius", "min_neighbours": "radius"}


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Statistical / radius outlier removal of a PLY point cloud (MI355X engine)")
    p.add_argument("src", metavar="IN.ply")
    p.add_argument("dst", metavar="OUT.ply")
    p.add_argument("--method", default="statistical", choices=["statistical", "radius"])
    p.add_argument("--k", type=int, default=None, help="statistical: neighbours per vertex, 1 .. 32 (default 20)")
    p.add_argument("--std_ratio", type=float, default=None, help="statistical: standard deviations above the mean (default 2.0)")
    p.add_argument("--max_dist", type=float, default=None,
                   help="statistical: how far the neighbour search looks, in world units (default: 0.02 x the diagonal of the "
                        "cloud's 1 %% .. 99 %% quantile box)")
    p.add_argument("--radius", type=float, default=None, help="radius: the radius in world units (no default)")
    p.add_argument("--min_neighbours", type=int, default=None, help="radius: other vertices needed within the radius (default 2)")
    p.add_argument("--device", default="cuda")
    return p


def check_args(args) -> None:
    """an option of the other method, radius without --radius and a value out of range are argparse errors (exit status 2)"""
    from itermvs_amd import cloud_filter
    error = build_parser().error
    for o in OPTIONS:
        if getattr(args, o) is not None and OWNER[o] != args.method:
            error("--{} belongs to --method {}, got --method {}".format(o, OWNER[o], args.method))
    if args.method == "radius" and args.radius is None:
        error("--method radius needs --radius (world units; there is no default)")
    problem = cloud_filter.method_problem(args.method, *[getattr(args, o) for o in OPTIONS])
    if problem:
        error("--method {}: --{}".format(args.method, problem))
    if os.path.abspath(args.src) == os.path.abspath(args.dst):
        error("OUT.ply must not be IN.ply")


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    check_args(args)
    from itermvs_amd import cloud_filter
    info = {}
    fn = cloud_filter.mask_function(args.method, *[getattr(args, o) for o in OPTIONS], device=args.device, info=info)
    got = cloud_filter.clean_ply(args.src, args.dst, fn)
    print("{}: {} vertices, kept {}, removed {} ({} of them not finite)".format(
        args.src, got["vertices"], got["kept"], got["removed"], info.get("non_finite", 0)))
    if args.method == "statistical" and got["vertices"]:
        print("statistical: k {} cap {:.6g} isolated {} mean {:.6g} std {:.6g} threshold {:.6g}; cell edge {:.6g}, {} queries on "
              "the coarse grid".format(20 if args.k is None else args.k, info["cap"], info["isolated"], info["mean"], info["std"],
                                       info["threshold"], info["edge"] or 0.0, info["second_pass"]))
    elif got["vertices"]:
        print("radius: r {:.6g} min_neighbours {}; cell edge {:.6g}".format(
            args.radius, 2 if args.min_neighbours is None else args.min_neighbours, info["edge"] or 0.0))
    print("seconds: sort {:.3f} search {:.3f}".format(info.get("seconds_sort", 0.0), info.get("seconds_search", 0.0)))
    print("wrote {}".format(args.dst))
    return dict(got, **info)


if __name__ == "__main__":
    main()
