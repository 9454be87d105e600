"""``eval.py --dataset folder --filter --fuse_source memory``: every scan goes from its image files to its point cloud in one
pass, fused from GPU memory.

The two-pass driver (``save_depth`` then ``fuse_scans`` -> ``fusion.filter_depth``) shares nothing but the disk between its
passes: the filter opens every image again (original size for the intrinsics scale; for reference views a second decode and
a Pillow resize for the vertex colours), reads every PFM back and uploads all of it before ``fusion.fuse_scan`` starts.
While the depth maps were computed, all of that was on the GPU already.  Here a scan's results stay there until its last
view is done:

  * ``depths_upsampled`` / ``confidence_upsampled`` of every view are copied out of the forward's static buffers into per-view
    device tensors, on the forward's stream, before the next forward overwrites them;
  * the colours of every reference view are ``ops.resize_rgb8`` (Pillow's bilinear resize, bit for bit) of the uint8 upload
    the input side makes anyway -- one decode gives the features and the colours;
  * the original image size (intrinsics scale) comes from that decode; no image file is opened for it and no PFM is read;
  * after the last view ``fusion.fuse_scan`` runs on the device tensors, and the scan's storage is dropped.

The forward is the one of today's loops: ``scan_dataset.Prefetcher`` + ``Pipeline.forward`` without ``--feature_cache``,
``scan_cache.ScanFeatureCache`` with ``plan_schedule`` over the scan's depth maps with it; same ``--projection host_fp32``
handling, deferred NaN-camera check, ``Iter`` lines and software-pipelined PFM writes (``--no_pfm`` skips the files).  The
PLY is byte for byte the one ``--fuse_points device`` writes from the files.  Ranks take whole scans: a scan's maps must
be on one GPU.

Memory: 11 bytes per pixel and view (two float32 maps and three colour bytes), about 1 GB for a 49-view scan at 1600 x 1152,
held until that scan is fused (the vertex records of ``fuse_scan`` come on top, as in the two-pass path).
"""
from __future__ import annotations

import os
import time
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import fusion, ops
from .data_io import save_pfm
from .scan_cache import ScanFeatureCache, _Decoder, _map_views, plan_schedule
from .scan_dataset import Prefetcher, to_device

NAN_CAMERA = "nan in proj (singular or non-finite camera matrix, module.py:83,87)"


class ColourPrefetcher(Prefetcher):
    """``Prefetcher`` whose staged item also carries ``sample['rgb']``: the reference view's bytes resized to the inference
    size like Pillow does (uint8 [H,W,3] on the device), from the same upload, on the same side stream, under the same
    ``ready`` event"""

    def _to_device(self, s):
        kept = {}
        tensors = to_device(s, self.dev, keep=kept)
        w, h = s["img_wh"]
        s["rgb"] = ops.resize_rgb8(kept["raw"][:1], h, w)[0]
        return tensors


class _ResultWriter:
    """the result side of ``save_depth_folder``, one depth map behind the GPU: forward n's downloads (its two maps unless
    ``no_pfm``, the engine's NaN-camera flag always) are enqueued, then the host checks and writes map n - 1"""

    def __init__(self, args, model, total: int):
        self.args, self.model, self.total = args, model, total
        self.no_pfm = bool(getattr(args, "no_pfm", False))
        self.host = [None, None]
        self.events = [torch.cuda.Event(), torch.cuda.Event()]
        self.prev = None
        self.n = 0

    def _finish(self, job) -> None:
        name, k, n, t0 = job
        self.events[k].synchronize()
        depth, conf, flag = self.host[k]
        if int(flag[0]) != 0:
            raise AssertionError(NAN_CAMERA)
        print("Iter {}/{}, time = {:.3f}".format(n, self.total, time.time() - t0))
        if not self.no_pfm:
            save_pfm(os.path.join(self.args.outdir, name.format("depth_est", ".pfm")), np.squeeze(depth.numpy()[0], 0))
            save_pfm(os.path.join(self.args.outdir, name.format("confidence", ".pfm")), np.squeeze(conf.numpy()[0], 0))

    def push(self, name: str, d: torch.Tensor, c: torch.Tensor, t0: float) -> None:
        k = self.n % 2
        if self.host[k] is None or self.host[k][0].shape != d.shape:
            self.host[k] = (torch.empty(d.shape, dtype=d.dtype).pin_memory(), torch.empty(c.shape, dtype=c.dtype).pin_memory(),
                            torch.zeros((1,), dtype=torch.int32).pin_memory())
        if not self.no_pfm:
            self.host[k][0].copy_(d, non_blocking=True)
            self.host[k][1].copy_(c, non_blocking=True)
        flag = self.model.projection_flag()
        if flag is not None:
            self.host[k][2].copy_(flag, non_blocking=True)
        self.events[k].record()
        if self.prev is not None:
            self._finish(self.prev)
        self.prev = (name, k, self.n, t0)
        self.n += 1

    def flush(self) -> None:
        if self.prev is not None:
            prev, self.prev = self.prev, None
            self._finish(prev)


class _ScanStore:
    """what one scan leaves on the GPU until it is fused: per view its depth map (and original image size), per reference
    view its confidence map and colours"""

    def __init__(self, pairs):
        self.refs = {ref for ref, _ in pairs}
        self.depth: Dict[int, torch.Tensor] = {}
        self.conf: Dict[int, torch.Tensor] = {}
        self.rgb: Dict[int, torch.Tensor] = {}
        self.size: Dict[int, Tuple[int, int]] = {}              # view -> (original_w, original_h)

    def keep_maps(self, view: int, d: torch.Tensor, c: torch.Tensor) -> None:
        """copies on the current stream: the forward's buffers are overwritten by the next one"""
        self.depth[view] = d[0, 0].clone()
        if view in self.refs:
            self.conf[view] = c[0, 0].clone()

    def keep_size(self, view: int, raw: torch.Tensor) -> None:
        self.size[view] = (int(raw.shape[-2]), int(raw.shape[-3]))


def scan_indices(dataset, scan: str) -> List[int]:
    return [i for i, m in enumerate(dataset.metas) if m[0] == scan]


def check_views(dataset, scan: str, pairs) -> None:
    """every view ``pair.txt`` names must get a depth map in this run, i.e. be a reference view of the scan (the two-pass
    path fails on the missing PFM); nothing is guessed"""
    have = {m[1] for m in dataset.metas if m[0] == scan}
    for ref, srcs in pairs:
        for v in (ref, *srcs):
            if v not in have:
                raise FileNotFoundError(f"{scan}: pair.txt names view {v} (a source of reference view {ref}) that is never a "
                                        f"reference view, so it has no depth map ({scan}/depth_est/{v:0>8}.pfm)")


def _forward_plain(args, dataset, indices, model, dev, store: _ScanStore, results: _ResultWriter) -> None:
    """``save_depth_folder``'s forward over one scan"""
    for (sample, (imgs, projs, dmin, dmax)), idx in zip(ColourPrefetcher(dataset, indices, dev), indices):
        t0 = time.time()
        _, ref, srcs = dataset.metas[idx]
        if model.projection == "host_fp32":
            projs = {key: v.unsqueeze(0) for key, v in sample["proj_matrices"].items()}      # CPU cameras
        out = model(imgs, projs, dmin, dmax)
        d, c = out["depths_upsampled"], out["confidence_upsampled"]
        store.keep_maps(ref, d, c)
        for v in [ref] + list(srcs[:dataset.nviews - 1]):
            store.keep_size(v, sample["raw"])
        if ref in store.refs:
            sample["rgb"].record_stream(torch.cuda.current_stream(dev))     # made on the prefetcher's stream, read by the fusion
            store.rgb[ref] = sample["rgb"]
        results.push(sample["filename"], d, c, t0)


def _forward_cached(args, dataset, indices, model, dev, cache: ScanFeatureCache, store: _ScanStore,
                    results: _ResultWriter) -> None:
    """``save_depth_cached``'s forward over one scan: the schedule is planned over this scan's depth maps"""
    w, h = dataset.img_wh
    maps = []
    for i in indices:
        scan, views = _map_views(dataset, i)
        maps.append([(scan, v) for v in views])
    steps = plan_schedule(maps, int(args.feature_cache), dataset.nviews)
    for item, idx, step in zip(_Decoder(dataset, indices, steps, dev), indices, steps):
        t0 = time.time()
        ref = dataset.metas[idx][1]
        if len(step.views) == 1:                   # no source view: exactly the uncached forward (its result or its error)
            s = dataset[idx]
            kept = {}
            imgs, projs, dmin, dmax = to_device(s, dev, keep=kept)
            if model.projection == "host_fp32":
                projs = {key: v.unsqueeze(0) for key, v in s["proj_matrices"].items()}
            out = model(imgs, projs, dmin, dmax)
            d, c = out["depths_upsampled"], out["confidence_upsampled"]
            store.keep_size(ref, kept["raw"])
            if ref in store.refs and ref not in store.rgb:
                store.rgb[ref] = ops.resize_rgb8(kept["raw"][:1], h, w)[0]
        else:
            eng, slab = cache.bind(h, w)
            if step.compute:
                raw = item["raw"].to(dev, non_blocking=True)
                x = ops.image_pyramid(raw, h, w, all_levels=False)["level_0"]
                cache.fill(step.compute, x)
                for j, ((_, vid), _) in enumerate(step.compute):
                    store.keep_size(vid, raw)
                    if vid in store.refs and vid not in store.rgb:      # kept until the scan is fused, whatever the cache evicts
                        store.rgb[vid] = ops.resize_rgb8(raw[j:j + 1], h, w)[0]
            pm = {l: item["proj_matrices"][f"level_{l}"].float().unsqueeze(0) for l in (1, 2, 3)}
            dmin = item["depth_min"].view(1).to(dev, non_blocking=True)
            dmax = item["depth_max"].view(1).to(dev, non_blocking=True)
            composed = None
            if model.projection == "host_fp32":
                composed = eng.compose_host(torch.stack([pm[1], pm[2], pm[3]]))
                assert not bool(torch.isnan(composed).any()), NAN_CAMERA
                projs = None
            else:
                projs = {l: t.to(dev, non_blocking=True) for l, t in pm.items()}
            d, c = cache.match(step.slots[0], step.slots[1:], projs, dmin, dmax, composed=composed)
        store.keep_maps(ref, d, c)
        results.push(item["filename"], d, c, t0)


def scan_cameras(scan_folder: str, views: Sequence[int], sizes: Dict[int, Tuple[int, int]], img_wh) -> dict:
    """cams[view] = (K, E) with the intrinsics rescaled to the depth maps' size by the function ``fusion.filter_depth`` uses;
    sizes[view] = (original_w, original_h)"""
    return {v: fusion.read_scaled_camera(scan_folder, v, img_wh[0] / sizes[v][0], img_wh[1] / sizes[v][1]) for v in views}


def fuse_scans_from_memory(args, dataset, scans: Sequence[str], model, dev) -> Dict[str, Dict[int, Tuple[float, float, float]]]:
    """depth maps and point clouds of ``scans`` (this rank's, whole scans) in one pass; ``dataset``: the
    ``ScanFolderDataset`` of the run, ``model``: the test-mode ``Pipeline`` on ``dev``.
    -> {scan: {ref_view: (geo, photo, final mask share)}}, the lines ``fuse_scans`` prints are printed as well."""
    dev = torch.device(dev)
    cache_n = int(getattr(args, "feature_cache", 0) or 0)
    img_wh = tuple(dataset.img_wh)
    pairs_of = {}
    for scan in scans:                                  # before any work: a scan that cannot be fused stops the run here
        pairs_of[scan] = fusion.read_pair_file(os.path.join(dataset.datapath, scan, "pair.txt"))
        check_views(dataset, scan, pairs_of[scan])
    indices_of = {scan: scan_indices(dataset, scan) for scan in scans}
    results = _ResultWriter(args, model, sum(len(v) for v in indices_of.values()))
    cache = ScanFeatureCache(model, cache_n) if cache_n > 0 else None
    model.check_nan = False                             # the flag travels with the results instead of stalling the stream
    os.makedirs(args.outdir, exist_ok=True)
    stats = {}
    with torch.no_grad():
        for scan in scans:
            pairs = pairs_of[scan]
            store = _ScanStore(pairs)
            if cache is not None:
                _forward_cached(args, dataset, indices_of[scan], model, dev, cache, store, results)
            else:
                _forward_plain(args, dataset, indices_of[scan], model, dev, store, results)
            results.flush()                             # the last map's NaN-camera check (and PFMs) before the scan is fused
            views = sorted({v for ref, srcs in pairs for v in (ref, *srcs)})
            cams = scan_cameras(os.path.join(dataset.datapath, scan), views, store.size, img_wh)
            mask_folder = os.path.join(args.outdir, scan, "mask") if getattr(args, "save_masks", False) else None
            stats[scan] = fusion.fuse_scan(pairs, cams, store.depth, store.conf, store.rgb,
                                           os.path.join(args.outdir, scan + ".ply"), device=str(dev), mask_folder=mask_folder,
                                           **fusion.fuse_keywords_from_args(args, os.path.join(args.outdir, scan + "_mesh.ply")))
            fusion.print_view_shares(scan, stats[scan])
            del store
    return stats
