#!/usr/bin/env python3
"""Depth inference driver -- counterpart of the reference's ``eval.py`` ``save_depth()`` (eval.py:104-151)
for the MI355X engine.  Same flags, checkpoint format and output layout
(``<outdir>/<scan>/depth_est/<view:08d>.pfm`` and ``.../confidence/...``), one process per GPU:

    python eval.py --dataset synthetic --n_views 5 --img_wh 640 512 --outdir ./outputs [--loadckpt model.ckpt]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 eval.py ...

Each rank takes the reference views ``rank, rank + world, ...`` (no collective on the data path).
``--dataset module:Class`` accepts any dataset yielding the reference's sample dict
(datasets/dtu_yao_eval.py:154-158); the reference's own loaders (cv2 / PIL based) are outside this
repository's scope.  ``--filter`` runs the reference's filter / fusion stage (eval.py:215-325) afterwards: for every scan
folder under ``--testpath`` that has a ``pair.txt``, ``cams_1/`` and ``images/``, the depth / confidence PFMs written above
are fused into ``<outdir>/<scan>.ply`` by ``itermvs_amd.fusion.filter_depth`` (one HIP launch per reference view); the
camera intrinsics are rescaled by ``--img_wh`` / original image size and the points coloured from the resized images like
eval.py:231-232,251-252,295.  ``--filter --fuse_source memory`` does both in one pass: each scan is fused from GPU memory when
its last depth map is done (``itermvs_amd.scan_fuse``), ``--no_pfm`` then leaves only the PLYs on the disk.
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from itermvs_amd import shard, synthetic  # noqa: E402
from itermvs_amd.data_io import save_pfm  # noqa: E402
from itermvs_amd.net import Pipeline  # noqa: E402


class _StoreGiven(argparse.Action):
    """store, and note on the namespace that the flag was given (``<dest>_given``): a default cannot be told from a typed value"""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + "_given", True)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Predict depth maps (MI355X engine)")
    p.add_argument("--model", default="IterMVS")
    p.add_argument("--dataset", default="synthetic",
                   help="'synthetic', 'folder' (scan folders under --testpath: pair.txt, cams_1/, images/; decode on the host, "
                        "normalise / resize / pyramid on the GPU, prefetched) or module:Class of an MVSDataset")
    p.add_argument("--testpath")
    p.add_argument("--testlist")
    p.add_argument("--split", default="intermediate")
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--n_views", type=int, default=5)
    p.add_argument("--img_wh", nargs="+", type=int, default=[640, 512], help="width height")
    p.add_argument("--loadckpt", default=None)
    p.add_argument("--outdir", default="./outputs")
    p.add_argument("--display", action="store_true")
    p.add_argument("--iteration", type=int, default=4)
    p.add_argument("--projection", default="device_fp64", choices=["device_fp64", "host_fp32"],
                   help="how src_proj @ inverse(ref_proj) (module.py:77-90) is composed: on the GPU in fp64 rounded once (default), or "
                        "on the host in fp32 operation for operation like the reference (tap indices of a reference run on this "
                        "host); the cameras then stay on the host, no synchronisation")
    p.add_argument("--conv_arithmetic", default="bf16x3", choices=["bf16x3", "fp32"],
                   help="3x3 convolutions with more than 8 input channels: exact three-term bf16 split of both operands on the bf16 "
                        "matrix instructions (default, fp32-rounding-class error) or the exact fp32 MFMA (bit-for-bit an fmaf chain)")
    p.add_argument("--feature_dtype", default="fp32", choices=["fp32", "bf16", "fp16"],
                   help="storage type of the feature pyramids (BASELINE cfg 5: fp16); arithmetic stays fp32")
    p.add_argument("--no_graphs", action="store_true",
                   help="launch every kernel from Python (~85 launches per depth map) instead of replaying one hipGraph per depth map "
                        "(captured once per image shape; results are bit-identical)")
    p.add_argument("--feature_cache", type=int, default=0,
                   help="--dataset folder only: keep the feature pyramids of at most N images on the GPU and compute each image's "
                        "pyramid once while it stays cached, instead of once per depth map that reads it (scan mode, "
                        "itermvs_amd.scan_cache; ranks then take contiguous blocks of (scan, view)).  0 = off (default); "
                        "N must be >= n_views.  The PFMs are byte-identical to the run without it")
    p.add_argument("--geo_pixel_thres", type=float, default=1)
    p.add_argument("--geo_depth_thres", type=float, default=0.01)
    p.add_argument("--photo_thres", type=float, default=0.3)
    p.add_argument("--geo_mask_thres", type=int, default=3, action=_StoreGiven,
                   help="--filter: source views that must agree with a reference pixel (eval.py:323-324: the reference fuses DTU "
                        "with 4 and everything else with 3; the default 3 keeps this driver's clouds as they were)")
    p.add_argument("--geo_consistency", default="static", choices=["static", "dynamic"],
                   help="--filter: how the source views decide a reference pixel's geometric mask.  static (default): at least "
                        "--geo_mask_thres of them reproject within --geo_pixel_thres and --geo_depth_thres; every byte as before.  "
                        "dynamic: dynamic consistency checking (D2HC-RMVSNet) -- a source passes level n when it reprojects within "
                        "n * --dyn_pixel_step pixels and n * --dyn_depth_step of relative depth, and the pixel is kept at the "
                        "smallest level n of --dyn_levels that at least n sources pass: few views that agree tightly or many that "
                        "agree loosely, with no per-scene count (itermvs_fuse_depth_dynamic).  --geo_mask_thres must then not be "
                        "given; the depth average still uses --geo_pixel_thres and --geo_depth_thres")
    p.add_argument("--dyn_pixel_step", type=float, default=None,
                   help="--geo_consistency dynamic: pixels of reprojection error allowed per level (default 0.25; from memory of "
                        "the published code, unverified)")
    p.add_argument("--dyn_depth_step", type=float, default=None,
                   help="--geo_consistency dynamic: relative depth difference allowed per level, rounded to float32 (default "
                        "1/1300; from memory of the published code, unverified)")
    p.add_argument("--dyn_levels", type=int, nargs=2, default=None, metavar=("MIN", "MAX"),
                   help="--geo_consistency dynamic: the levels that are tried, 1 <= MIN <= MAX <= 16 (default 2 10; from memory of "
                        "the published code, unverified); levels above the number of source views cannot accept")
    p.add_argument("--num_samples", type=int, default=8, help="synthetic dataset: number of reference views")
    p.add_argument("--filter", action="store_true", help="fuse the saved depth maps of every scan into a point cloud (eval.py:311-325)")
    p.add_argument("--fuse_points", default="host", choices=["host", "device"],
                   help="--filter with --fuse_source files: where the surviving pixels become PLY vertices (eval.py:287-308): numpy "
                        "on the host with one synchronisation per reference view (default), or itermvs_fuse_points on the GPU with "
                        "one per group of views.  --fuse_source memory always assembles the vertex records on the GPU")
    p.add_argument("--fuse_source", default="files", choices=["files", "memory"],
                   help="--filter: what the fusion reads.  files (default): the PFMs and images, in a second pass after every depth "
                        "map is written.  memory (needs --dataset folder): each scan is fused from GPU memory as soon as its last "
                        "depth map is done -- no PFM is read back and no image is decoded twice (itermvs_amd.scan_fuse; ranks "
                        "take whole scans; the PLY is byte for byte the one of --fuse_points device)")
    p.add_argument("--fuse_dedupe", action="store_true",
                   help="--filter with the point cloud assembled on the GPU (--fuse_points device or --fuse_source memory): emit each "
                        "surface point once per scan.  A pixel that an emitted point of an earlier reference view was verified against "
                        "(the nearest pixel of a consistent reprojection, unless it lies across a depth edge) is dropped from its own "
                        "view's vertices; what remains is a sub-sequence of the default cloud.  Off (default): every byte as before")
    p.add_argument("--ply_normals", action="store_true",
                   help="--filter with the point cloud assembled on the GPU (--fuse_points device or --fuse_source memory): every "
                        "PLY vertex carries nx ny nz between z and red (the layout of COLMAP's fused.ply), the unit normal of the "
                        "surface at the pixel: the cross product of the fused depth map's differences to the neighbouring pixels "
                        "along the row and the column, in world space, facing the reference camera that saw the point; (0, 0, 0) "
                        "where no neighbour on the same surface exists.  Off (default): every byte as before")
    p.add_argument("--normal_edge_thres", type=float, default=0.01,
                   help="--ply_normals: a neighbouring pixel whose fused depth differs by this share of the pixel's depth or more "
                        "lies across a depth edge and is not used for the normal.  The default is the step --geo_depth_thres "
                        "already treats as another surface (at 640 px wide it still admits surfaces slanted by about 85 degrees); "
                        "a choice, not a measured optimum")
    p.add_argument("--mesh", action="store_true",
                   help="--filter with the point cloud assembled on the GPU (--fuse_points device or --fuse_source memory): also write "
                        "<outdir>/<scan>_mesh.ply, a coloured triangle mesh.  Every reference view's fused depth map is integrated into "
                        "a dense truncated-signed-distance volume on the GPU (itermvs_tsdf_integrate) and marching tetrahedra turns it "
                        "into triangles (itermvs_tsdf_mesh); the same inputs give the same bytes.  Off (default): every byte as before")
    p.add_argument("--mesh_resolution", type=int, default=256,
                   help="--mesh: voxels along the longest side of the bounds (ignored with --mesh_voxel).  The default is a choice: "
                        "a 256-cube of 12-byte voxels takes 0.2 GB, 512 takes 1.6 GB, plus as much again while the triangles are extracted")
    p.add_argument("--mesh_voxel", type=float, default=None, help="--mesh: the voxel's side in world units, instead of --mesh_resolution")
    p.add_argument("--mesh_bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                   help="--mesh: the volume in world units, used as given.  Default: per axis the --mesh_bounds_quantile and 1 - quantile "
                        "order statistics of the fused cloud's vertices, widened by the truncation distance")
    p.add_argument("--mesh_bounds_quantile", type=float, default=0.01,
                   help="--mesh without --mesh_bounds: share of the cloud's vertices left outside the volume at either end of each "
                        "axis, in [0, 0.5).  The default keeps a few stray points from inflating the volume; a choice, not a measured optimum")
    p.add_argument("--mesh_trunc", type=float, default=3.0,
                   help="--mesh: truncation distance of the signed distance in voxels, at least 1.  The default spans the depth noise "
                        "of a few voxels without bridging thin gaps; a choice, not a measured optimum")
    p.add_argument("--mesh_min_count", type=int, default=2,
                   help="--mesh: views that must have seen a voxel before it takes part in a triangle.  The default asks a second view "
                        "to confirm free or occupied space; a choice, not a measured optimum")
    p.add_argument("--mesh_min_component", type=int, default=None, metavar="N",
                   help="--mesh: leave the connected components of the mesh with fewer than N triangles out of <scan>_mesh.ply "
                        "(floating fragments; found and removed on the GPU before the download).  No default: without this flag and "
                        "--mesh_component_share every triangle is written, as before")
    p.add_argument("--mesh_component_share", type=float, default=None, metavar="F",
                   help="--mesh: leave out the components with fewer than F x the triangles of the largest component, F in [0, 1]: "
                        "a threshold without a scale.  With --mesh_min_component a component must pass both.  No default")
    p.add_argument("--mesh_simplify", type=float, default=None, metavar="F",
                   help="--mesh: also write <outdir>/<scan>_mesh_simplified.ply, the mesh of <scan>_mesh.ply (after the component "
                        "filter, if that is on) simplified on the GPU by vertex clustering with quadric placement: one vertex per "
                        "occupied cell of F voxels' side, placed at the minimiser of the cell's plane quadrics, so corners and planes "
                        "stay.  <scan>_mesh.ply and every other output byte stay as they are.  No default; 2 is a reasonable start "
                        "(marching tetrahedra emit triangles far smaller than the depth noise)")
    p.add_argument("--mesh_budget_gb", type=float, default=16.0,
                   help="--mesh: GPU memory in GiB that the kept fused views (9 bytes per pixel and view), the volume, the extraction "
                        "workspace, the mesh buffers, the component filter's labels, counts and workspace and the simplifier's keys, "
                        "sort orders, representatives and workspace may take together; a larger request stops with the bytes it needs.  A choice")
    p.add_argument("--clean_cloud", default=None, choices=["statistical", "radius"],
                   help="--filter: also write <outdir>/<scan>_clean.ply, the scan's cloud without its outliers (floaters: sky pixels, "
                        "specular surfaces, thin structures that pass the masks in a few views); <scan>.ply and every other output "
                        "stay byte for byte as without the flag, the kept vertex records are copied unchanged and in order.  "
                        "statistical: a vertex goes when the mean distance to its --clean_k nearest neighbours exceeds the cloud's "
                        "mean of that distance by --clean_std_ratio standard deviations, or fewer than k vertices lie within "
                        "--clean_max_dist (Open3D's remove_statistical_outlier; itermvs_cloud_knn_mean).  radius: a vertex goes when "
                        "fewer than --clean_min_neighbours others lie within --clean_radius (itermvs_cloud_radius_count)")
    p.add_argument("--clean_k", type=int, default=None, help="--clean_cloud statistical: neighbours per vertex, 1 .. 32 (default 20, "
                                                              "Open3D's usual value; not a measured optimum)")
    p.add_argument("--clean_std_ratio", type=float, default=None,
                   help="--clean_cloud statistical: standard deviations above the mean (default 2.0, Open3D's usual value; not a "
                        "measured optimum)")
    p.add_argument("--clean_max_dist", type=float, default=None,
                   help="--clean_cloud statistical: how far the neighbour search looks, in world units (default: 0.02 x the diagonal "
                        "of the cloud's 1 %% .. 99 %% quantile box; a choice, not a measured optimum)")
    p.add_argument("--clean_radius", type=float, default=None, help="--clean_cloud radius: the radius in world units (no default)")
    p.add_argument("--clean_min_neighbours", type=int, default=None,
                   help="--clean_cloud radius: other vertices a vertex needs within the radius (default 2)")
    p.add_argument("--no_pfm", action="store_true",
                   help="--fuse_source memory only: do not write the depth / confidence PFMs, only the PLY (and the masks of "
                        "--save_masks) reaches the disk")
    p.add_argument("--save_masks", action="store_true",
                   help="--filter: write <outdir>/<scan>/mask/<view>_photo.png, _geo.png, _final.png like the reference (eval.py:266-269)")
    return p


class SyntheticMVSDataset(torch.utils.data.Dataset):
    """Photo-consistent synthetic scenes in the reference's sample-dict schema."""

    def __init__(self, n_views: int, img_wh, count: int):
        self.n_views, self.w, self.h, self.count = n_views, img_wh[0], img_wh[1], count

    def __len__(self):
        return self.count

    def __getitem__(self, idx):
        s = synthetic.make_scene_sample(num_views=self.n_views, height=self.h, width=self.w, seed=idx)
        return {"imgs": {k: v[0] for k, v in s["imgs"].items()},
                "proj_matrices": {k: v[0] for k, v in s["proj_matrices"].items()},
                "depth_min": s["depth_min"][0], "depth_max": s["depth_max"][0],
                "filename": "scan_synthetic/{}/" + "{:0>8}".format(idx) + "{}"}


def scan_list(args):
    """--testlist (one scan folder name per line, eval.py:47 of the reference) or every folder of --testpath with a pair.txt"""
    if args.testlist:
        with open(args.testlist) as f:
            return [line.rstrip() for line in f if line.strip()]
    return sorted(d for d in os.listdir(args.testpath) if os.path.isfile(os.path.join(args.testpath, d, "pair.txt")))


def make_dataset(args):
    if args.dataset == "synthetic":
        return SyntheticMVSDataset(args.n_views, args.img_wh, args.num_samples)
    if args.dataset == "folder":
        from itermvs_amd.scan_dataset import ScanFolderDataset
        return ScanFolderDataset(args.testpath, scan_list(args), args.n_views, tuple(args.img_wh))
    mod, cls = args.dataset.split(":")
    return getattr(importlib.import_module(mod), cls)(args.testpath, args.testlist, args.n_views, tuple(args.img_wh))


def collate(samples):
    out = {"imgs": {}, "proj_matrices": {}}
    for key in ("imgs", "proj_matrices"):
        for lvl in samples[0][key]:
            out[key][lvl] = torch.stack([torch.as_tensor(s[key][lvl]) for s in samples])
    out["depth_min"] = torch.stack([torch.as_tensor(s["depth_min"], dtype=torch.float32) for s in samples])
    out["depth_max"] = torch.stack([torch.as_tensor(s["depth_max"], dtype=torch.float32) for s in samples])
    out["filename"] = [s["filename"] for s in samples]
    return out


def tocuda(x, dev):
    """utils.py:60-67"""
    if isinstance(x, torch.Tensor):
        return x.to(dev, non_blocking=True)
    if isinstance(x, dict):
        return {k: tocuda(v, dev) for k, v in x.items()}
    return x


def load_model(args, dev) -> Pipeline:
    model = Pipeline(iteration=args.iteration, test=True)
    model.feature_dtype = getattr(args, "feature_dtype", "fp32")
    model.projection = getattr(args, "projection", "device_fp64")
    model.conv_arithmetic = getattr(args, "conv_arithmetic", "bf16x3")
    # one hipGraph replay per depth map (bit-identical to the eager launches); host_fp32 with device-resident cameras cannot be
    # captured -- save_depth keeps the cameras on the host for that mode
    model.use_graphs = not getattr(args, "no_graphs", False)
    # which arithmetic produced the PFMs of this run (device_fp64 moves ~1e-5 of the tap floors against the reference's host fp32
    # composition; host_fp32 follows module.py:77-90 operation for operation)
    print("depth maps: projection = {}, conv arithmetic = {}, feature storage = {}".format(
        model.projection, model.conv_arithmetic, model.feature_dtype))
    if args.loadckpt:
        print("loading model {}".format(args.loadckpt))
        state = torch.load(args.loadckpt, map_location="cpu", weights_only=False)
        model.load_checkpoint_state(state["model"])            # eval.py:124-125 ('module.' prefixed keys)
    else:
        model.load_state_dict(synthetic.random_state_dict(0))
    return model.to(dev).eval()


def check_feature_cache(args) -> int:
    """--feature_cache N: 0 = off; N > 0 needs --dataset folder and N >= n_views"""
    n = int(getattr(args, "feature_cache", 0) or 0)
    if n < 0:
        raise SystemExit(f"--feature_cache must be >= 0, got {n}")
    if n > 0 and args.dataset != "folder":
        raise SystemExit(f"--feature_cache {n} needs --dataset folder (scan folders with pair.txt), got --dataset {args.dataset}")
    if n > 0 and n < args.n_views:
        raise SystemExit(f"--feature_cache {n} is below --n_views {args.n_views}: a depth map's views must fit in the cache")
    return n


def check_fuse_source(args) -> str:
    """--fuse_source memory needs --dataset folder and --filter; --no_pfm needs --fuse_source memory"""
    source = getattr(args, "fuse_source", "files")
    if source == "memory":
        missing = [flag for flag, ok in (("--dataset folder", args.dataset == "folder"), ("--filter", bool(args.filter))) if not ok]
        if missing:
            raise SystemExit("--fuse_source memory needs {} (scan folders with pair.txt, fused as their depth maps finish), got "
                             "--dataset {}{}".format(" and ".join(missing), args.dataset, "" if args.filter else " without --filter"))
    if getattr(args, "no_pfm", False) and source != "memory":
        raise SystemExit("--no_pfm needs --fuse_source memory: --fuse_source files fuses the PFMs it would skip")
    return source


def _check_gpu_assembly_flag(args, name: str, flag: str, why: str) -> bool:
    """a flag of the GPU point assembly needs --filter and --fuse_points device or --fuse_source memory"""
    if not getattr(args, name, False):
        return False
    on_gpu = getattr(args, "fuse_points", "host") == "device" or getattr(args, "fuse_source", "files") == "memory"
    missing = [f for f, ok in (("--filter", bool(args.filter)), ("--fuse_points device or --fuse_source memory", on_gpu))
               if not ok]
    if missing:
        raise SystemExit("{} needs {} ({}), got {}--fuse_points {} "
                         "--fuse_source {}".format(flag, " and ".join(missing), why, "" if args.filter else "no --filter, ",
                                                   getattr(args, "fuse_points", "host"), getattr(args, "fuse_source", "files")))
    return True


def check_fuse_dedupe(args) -> bool:
    """--fuse_dedupe needs --filter and the GPU point assembly (--fuse_points device or --fuse_source memory)"""
    return _check_gpu_assembly_flag(args, "fuse_dedupe", "--fuse_dedupe", "the claim maps live on the GPU while a scan is fused")


def check_ply_normals(args) -> bool:
    """--ply_normals needs --filter and the GPU point assembly, and --normal_edge_thres a finite value above 0"""
    if not _check_gpu_assembly_flag(args, "ply_normals", "--ply_normals",
                                    "the normals are computed on the GPU while the vertices are emitted"):
        return False
    edge = getattr(args, "normal_edge_thres", 0.01)
    if not 0 < edge < float("inf"):
        raise SystemExit(f"--normal_edge_thres must be a finite share of the depth above 0, got {edge}")
    return True


def check_mesh(args) -> bool:
    """--mesh needs --filter and the GPU point assembly; its numeric flags are checked where the options are built, before any work.
    --mesh_min_component, --mesh_component_share and --mesh_simplify need --mesh: an argparse error (usage, exit status 2) without it,
    like a --mesh_simplify that is not above 0"""
    if not getattr(args, "mesh", False):
        for flag in ("mesh_min_component", "mesh_component_share"):
            if getattr(args, flag, None) is not None:
                build_parser().error("--{} needs --mesh (it filters the mesh's connected components)".format(flag))
        if getattr(args, "mesh_simplify", None) is not None:
            build_parser().error("--mesh_simplify needs --mesh (it simplifies the mesh of <scan>_mesh.ply)")
    if getattr(args, "mesh_simplify", None) is not None and not 0.0 < args.mesh_simplify < float("inf"):
        build_parser().error("--mesh_simplify must be a finite cell side in voxels above 0, got {}".format(args.mesh_simplify))
    if not _check_gpu_assembly_flag(args, "mesh", "--mesh", "the volume is integrated from the fused depth maps that stay on the GPU"):
        return False
    from itermvs_amd import fusion
    try:
        fusion.mesh_options_from_args(args, "mesh.ply")
    except ValueError as e:
        raise SystemExit("--" + str(e).replace("mesh: ", "mesh_", 1))
    return True


def check_geo_consistency(args) -> str:
    """--geo_consistency dynamic needs --filter, takes no --geo_mask_thres and checks its --dyn_* values; the --dyn_* flags need
    it.  What is refused is refused as an argparse error (usage, exit status 2), before any work."""
    from itermvs_amd import fusion
    mode = getattr(args, "geo_consistency", "static")
    given = [flag for flag in ("dyn_pixel_step", "dyn_depth_step", "dyn_levels") if getattr(args, flag, None) is not None]
    error = build_parser().error
    if mode != "dynamic":
        if given:
            error("--{} needs --geo_consistency dynamic".format(given[0]))
        return mode
    if not args.filter:
        error("--geo_consistency dynamic needs --filter (it is a rule of the fusion stage)")
    if getattr(args, "geo_mask_thres_given", False):
        error("--geo_mask_thres {} cannot be given with --geo_consistency dynamic: the level rule takes the place of the count "
              "(see --dyn_levels)".format(args.geo_mask_thres))
    rule = fusion.consistency_from_args(args)
    problem = fusion.dynamic_problem(rule["dyn_pixel_step"], rule["dyn_depth_step"], rule["dyn_n_min"], rule["dyn_n_max"])
    if problem == "steps":
        error("--geo_consistency dynamic: --dyn_pixel_step and --dyn_depth_step (rounded to float32) must be finite and above 0, "
              "got {} and {}".format(rule["dyn_pixel_step"], rule["dyn_depth_step"]))
    if problem == "levels":
        error("--geo_consistency dynamic: --dyn_levels MIN MAX must satisfy 1 <= MIN <= MAX <= 16, got {}..{}".format(
            rule["dyn_n_min"], rule["dyn_n_max"]))
    return mode


CLEAN_OPTIONS = ("clean_k", "clean_std_ratio", "clean_max_dist", "clean_radius", "clean_min_neighbours")


def check_clean_cloud(args):
    """--clean_cloud needs --filter, radius needs --clean_radius, and a --clean_* option needs --clean_cloud: argparse errors
    (usage, exit status 2) before any work.  -> the method or None"""
    from itermvs_amd import cloud_filter
    method = getattr(args, "clean_cloud", None)
    error = build_parser().error
    given = [o for o in CLEAN_OPTIONS if getattr(args, o, None) is not None]
    if method is None:
        if given:
            error("--{} needs --clean_cloud".format(given[0]))
        return None
    if not args.filter:
        error("--clean_cloud needs --filter (it cleans the fused cloud of each scan)")
    if method == "radius" and getattr(args, "clean_radius", None) is None:
        error("--clean_cloud radius needs --clean_radius (world units; there is no default)")
    problem = cloud_filter.method_problem(method, *[getattr(args, o, None) for o in CLEAN_OPTIONS])
    if problem:
        error("--clean_cloud {}: --clean_{}".format(method, problem))
    return method


def clean_scan_cloud(args, scan: str, device) -> None:
    """--clean_cloud: <outdir>/<scan>.ply -> <outdir>/<scan>_clean.ply (itermvs_amd.cloud_filter); the cloud itself is only read"""
    from itermvs_amd import cloud_filter
    method = getattr(args, "clean_cloud", None)
    if method is None or not os.path.isfile(os.path.join(args.outdir, scan + ".ply")):
        return
    info = {}
    fn = cloud_filter.mask_function(method, *[getattr(args, o, None) for o in CLEAN_OPTIONS], device=device, info=info)
    got = cloud_filter.clean_ply(os.path.join(args.outdir, scan + ".ply"), os.path.join(args.outdir, scan + "_clean.ply"), fn)
    print("cleaning {} ({}): kept {} removed {} of {} vertices{}, sort {:.3f} s search {:.3f} s".format(
        scan, method, got["kept"], got["removed"], got["vertices"],
        ", isolated {} threshold {:.6g}".format(info.get("isolated", 0), info.get("threshold", float("nan")))
        if method == "statistical" else "", info.get("seconds_sort", 0.0), info.get("seconds_search", 0.0)))


def fuse_memory(args) -> dict:
    """--fuse_source memory: depth maps and point clouds in one pass (itermvs_amd.scan_fuse); scans are sharded over the
    ranks whole, like ``fuse_scans`` shards them.  -> {scan: {ref_view: (geo, photo, final mask share)}} of this rank"""
    from itermvs_amd.scan_fuse import fuse_scans_from_memory
    check_fuse_source(args)
    check_fuse_dedupe(args)
    check_ply_normals(args)
    check_mesh(args)
    check_geo_consistency(args)
    check_clean_cloud(args)
    check_feature_cache(args)
    rank, local_rank, world = shard.init_distributed()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dataset = make_dataset(args)
    model = load_model(args, dev)
    scans = list(dict.fromkeys(m[0] for m in dataset.metas))
    mine = [scans[i] for i in shard.shard_indices(len(scans), rank, world)]
    stats = fuse_scans_from_memory(args, dataset, mine, model, dev)
    for scan in mine:
        clean_scan_cloud(args, scan, dev)
    shard.barrier()
    return stats


def save_depth(args) -> int:
    cache_n = check_feature_cache(args)
    rank, local_rank, world = shard.init_distributed()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dataset = make_dataset(args)
    model = load_model(args, dev)
    if cache_n > 0:
        # scan mode: a contiguous block of (scan, view) per rank, so the rank's depth maps share their images
        from itermvs_amd.scan_cache import save_depth_cached
        done = save_depth_cached(args, dataset, shard.shard_contiguous(len(dataset), rank, world), model, dev)
        shard.barrier()
        return done
    mine = shard.shard_indices(len(dataset), rank, world)
    done = 0
    if args.dataset == "folder":
        return save_depth_folder(args, dataset, mine, model, dev)
    with torch.no_grad():
        for i in range(0, len(mine), args.batch_size):
            t0 = time.time()
            sample = collate([dataset[j] for j in mine[i:i + args.batch_size]])
            cu = tocuda(sample, dev)
            if model.projection == "host_fp32":
                cu["proj_matrices"] = sample["proj_matrices"]      # composed on the host: the cameras never need the device
            out = model(cu["imgs"], cu["proj_matrices"], cu["depth_min"], cu["depth_max"])
            depth = out["depths_upsampled"].cpu().numpy()      # D2H + sync, like tensor2numpy (eval.py:135)
            conf = out["confidence_upsampled"].cpu().numpy()
            model.check_projection_finite()                    # module.py:83,87 (deferred; the device is already idle)
            print("Iter {}/{}, time = {:.3f}".format(i // args.batch_size, (len(mine) + args.batch_size - 1) // args.batch_size,
                                                      time.time() - t0))
            for name, d, c in zip(sample["filename"], depth, conf):
                save_pfm(os.path.join(args.outdir, name.format("depth_est", ".pfm")), np.squeeze(d, 0))
                save_pfm(os.path.join(args.outdir, name.format("confidence", ".pfm")), np.squeeze(c, 0))
                done += 1
    shard.barrier()
    return done


def save_depth_folder(args, dataset, mine, model, dev) -> int:
    """the folder input side: a host thread decodes the next views while the GPU works; uint8 upload + pyramid kernel on a
    side stream (itermvs_amd.scan_dataset.Prefetcher); one reference view per forward like the reference's batch_size 1.
    The loop is software-pipelined by one depth map on ONE stream: forward n and the asynchronous download of its two maps
    (and of the engine's NaN flag, module.py:83,87) are enqueued, then the host writes the PFMs of map n-1 while the GPU
    works on n -- the reference's loop (eval.py:128-151) leaves the GPU idle for every file it writes."""
    from itermvs_amd.scan_dataset import Prefetcher
    done = 0
    host = [None, None]                                        # two sets of pinned result buffers, used alternately
    events = [torch.cuda.Event(), torch.cuda.Event()]
    model.check_nan = False                                    # the flag travels with the results instead of stalling the stream

    def finish(job) -> None:
        sample, k, n, t0 = job
        events[k].synchronize()                                # forward n-1 and its downloads are done; forward n is running
        depth, conf, flag = host[k]
        if int(flag[0]) != 0:
            raise AssertionError("nan in proj (singular or non-finite camera matrix, module.py:83,87)")
        print("Iter {}/{}, time = {:.3f}".format(n, len(mine), time.time() - t0))
        name = sample["filename"]
        save_pfm(os.path.join(args.outdir, name.format("depth_est", ".pfm")), np.squeeze(depth.numpy()[0], 0))
        save_pfm(os.path.join(args.outdir, name.format("confidence", ".pfm")), np.squeeze(conf.numpy()[0], 0))

    with torch.no_grad():
        prev = None
        for n, (sample, (imgs, projs, dmin, dmax)) in enumerate(Prefetcher(dataset, mine, dev)):
            t0 = time.time()
            if model.projection == "host_fp32":
                projs = {key: v.unsqueeze(0) for key, v in sample["proj_matrices"].items()}      # CPU cameras
            out = model(imgs, projs, dmin, dmax)
            k = n % 2
            d, c = out["depths_upsampled"], out["confidence_upsampled"]
            if host[k] is None or host[k][0].shape != d.shape:
                host[k] = (torch.empty(d.shape, dtype=d.dtype).pin_memory(), torch.empty(c.shape, dtype=c.dtype).pin_memory(),
                           torch.zeros((1,), dtype=torch.int32).pin_memory())
            host[k][0].copy_(d, non_blocking=True)
            host[k][1].copy_(c, non_blocking=True)
            flag = model.projection_flag()
            if flag is not None:
                host[k][2].copy_(flag, non_blocking=True)
            events[k].record()
            if prev is not None:
                finish(prev)
                done += 1
            prev = (sample, k, n, t0)
        if prev is not None:
            finish(prev)
            done += 1
    shard.barrier()
    return done


def fuse_scans(args) -> int:
    """eval.py:311-325: one point cloud per scan; scans are sharded over the ranks like the reference views"""
    from itermvs_amd import fusion
    check_fuse_dedupe(args)
    check_ply_normals(args)
    check_mesh(args)
    check_geo_consistency(args)
    check_clean_cloud(args)
    rank, local_rank, world = shard.init_distributed()
    dev = "cuda:%d" % local_rank
    scans = sorted(d for d in os.listdir(args.testpath)
                   if os.path.isfile(os.path.join(args.testpath, d, "pair.txt")) and os.path.isdir(os.path.join(args.outdir, d)))
    n = 0
    for i in shard.shard_indices(len(scans), rank, world):
        scan = scans[i]
        stats = fusion.filter_depth(os.path.join(args.testpath, scan), os.path.join(args.outdir, scan),
                                    os.path.join(args.outdir, scan + ".ply"), device=dev, img_wh=tuple(args.img_wh),
                                    points=args.fuse_points, save_masks=args.save_masks,
                                    **fusion.fuse_keywords_from_args(args, os.path.join(args.outdir, scan + "_mesh.ply")))
        fusion.print_view_shares(scan, stats)
        clean_scan_cloud(args, scan, dev)
        n += 1
    shard.barrier()
    return n


if __name__ == "__main__":
    a = build_parser().parse_args()
    print("argv:", sys.argv[1:])
    check_fuse_dedupe(a)
    check_ply_normals(a)
    check_mesh(a)
    check_geo_consistency(a)
    check_clean_cloud(a)
    if check_fuse_source(a) == "memory":
        fuse_memory(a)
    else:
        save_depth(a)
        if a.filter:
            fuse_scans(a)
