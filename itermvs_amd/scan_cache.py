"""Scan mode: each image's feature pyramid is computed once per scan and reused by every depth map that reads it.

The reference runs FeatureNet on all V views of every sample (models/net.py:52-65, called per sample from eval.py:128-133).
In a DTU scan an image is the reference view of one depth map and a source view of about four others
(datasets/dtu_yao_eval.py:25-34), so it goes through FeatureNet about five times.  Here a per-device slab of N image slots
(``engine.FeatureSlab``) keeps the pyramids; the correlation kernels read source views in place through a slot table
(itermvs_corr_iter_slots / itermvs_corr_init_slots) and one captured graph per (image shape, S, B) serves every reference
view (``engine.CachedRunner``).

Three parts:
  ``plan_schedule``  pure Python: a rank's ordered depth maps -> which images to compute before each map and where they go.
                     The list is known in advance, so eviction is exact (Belady): the cached image whose next use lies
                     furthest ahead leaves first.
  ``ScanFeatureCache``  the slab + the key -> slot map of one device, invalidated with the engine (weights, feature_dtype,
                     conv_arithmetic: ``Pipeline.invalidate``).
  ``save_depth_cached``  the driver loop of ``eval.py --dataset folder --feature_cache N``: a host thread decodes each image
                     once per computation, the uint8 upload + ``itermvs_image_pyramid`` + FeatureNet run into the slab,
                     then the matching graph replays.
"""
from __future__ import annotations

import os
import queue
import threading
import time
from typing import Dict, Hashable, List, NamedTuple, Sequence, Tuple

import numpy as np
import torch

Key = Hashable


class Step(NamedTuple):
    """what happens before depth map i: ``compute`` = [(key, slot)] images to run through FeatureNet (into these slots, evicted
    images already dropped), ``slots`` = the slot of every view of the map (reference first)"""
    views: Tuple[Key, ...]
    compute: Tuple[Tuple[Key, int], ...]
    slots: Tuple[int, ...]


def plan_schedule(maps: Sequence[Sequence[Key]], capacity: int, n_views: int) -> List[Step]:
    """``maps``: per depth map the keys of its views (reference first, at most ``n_views``) in the order they run.
    Returns one ``Step`` per map.  Every view of a map is resident when it runs; an image is computed again only after
    it was evicted; eviction takes the resident image whose next use is furthest away (never = infinitely far).
    Free slots are handed out lowest first, so the images of one map usually land in consecutive slots (one FeatureNet
    call).  A capacity below ``n_views`` is refused."""
    if n_views < 1:
        raise ValueError(f"n_views must be >= 1, got {n_views}")
    if capacity < n_views:
        raise ValueError(f"feature cache capacity {capacity} is below n_views = {n_views}: a depth map's views must fit")
    maps = [tuple(m) for m in maps]
    for m in maps:
        if len(m) > n_views or len(set(m)) != len(m):
            raise ValueError(f"a depth map has more than n_views = {n_views} views, or a view twice: {m}")
    # next use of every key after position i: walk backwards once
    uses: Dict[Key, List[int]] = {}
    for i, m in enumerate(maps):
        for k in m:
            uses.setdefault(k, []).append(i)
    ptr = {k: 0 for k in uses}                 # index into uses[k] of the first use >= current map
    resident: Dict[Key, int] = {}
    free = list(range(capacity))               # kept sorted: lowest slot first
    steps = []
    for i, m in enumerate(maps):
        for k in m:
            while uses[k][ptr[k]] < i:
                ptr[k] += 1
        missing = [k for k in m if k not in resident]
        need = len(missing) - len(free)
        if need > 0:
            def next_use(k):
                u, p = uses[k], ptr[k]
                while p < len(u) and u[p] <= i:
                    p += 1
                return u[p] if p < len(u) else float("inf")
            cands = sorted((k for k in resident if k not in m), key=lambda k: (-next_use(k), resident[k]))
            for k in cands[:need]:
                free.append(resident.pop(k))
            free.sort()
        compute = []
        for k in missing:
            slot = free.pop(0)
            resident[k] = slot
            compute.append((k, slot))
        steps.append(Step(m, tuple(compute), tuple(resident[k] for k in m)))
    return steps


class ScanFeatureCache:
    """``capacity`` image pyramids of one image size on the device of ``model`` (a test-mode ``Pipeline``).  The slab and the
    captured matching graphs belong to the engine that filled them: when ``model.inference_engine()`` returns another engine
    (new weights, ``feature_dtype`` / ``conv_arithmetic`` after ``invalidate``), every cached pyramid is dropped."""

    def __init__(self, model, capacity: int):
        if capacity < 1:
            raise ValueError("ScanFeatureCache: capacity must be >= 1")
        self.model, self.capacity = model, capacity
        self.engine = None
        self.slab = None
        self.resident: Dict[Key, int] = {}
        self.runners: Dict[tuple, object] = {}
        self.computed = 0                 # images run through FeatureNet (tests and tools/scan_bench.py read it)

    def bind(self, height: int, width: int):
        """the slab for images of ``height`` x ``width`` of the model's current engine (a new engine or size drops the contents)"""
        eng = self.model.inference_engine()
        if eng is not self.engine or self.slab is None or (self.slab.height, self.slab.width) != (height, width):
            self.engine, self.slab = eng, None
            self.resident, self.runners = {}, {}
            torch.cuda.synchronize(eng.device)          # the old slab may still be read by enqueued work
            self.slab = eng.new_slab(self.capacity, height, width)
        return self.engine, self.slab

    def fill(self, compute: Sequence[Tuple[Key, int]], images: torch.Tensor) -> None:
        """FeatureNet of ``images`` [K,3,H,W] (level 0 of the reference's pyramid) into the planned slots"""
        for k, slot in compute:
            for kk in [kk for kk, s in self.resident.items() if s == slot]:
                del self.resident[kk]
        self.engine.features_into(self.slab, images, [s for _, s in compute])
        for k, slot in compute:
            self.resident[k] = slot
        self.computed += len(compute)

    def match(self, ref_slot: int, src_slots: Sequence[int], projs, depth_min, depth_max, composed=None):
        """one depth map from cached pyramids (B = 1): the captured graph of (image shape, S) when the model uses graphs"""
        eng = self.engine
        s = len(src_slots)
        if not getattr(self.model, "use_graphs", False):
            return eng.run_cached(self.slab, [ref_slot], [list(src_slots)], projs, depth_min, depth_max,
                                  composed=None if composed is None else composed.to(eng.device, non_blocking=True))
        from .engine import CachedRunner
        key = (s, composed is not None)
        runner = self.runners.get(key)
        if runner is None:
            runner = self.runners[key] = CachedRunner(eng, self.slab, 1, s, host_composed=composed is not None)
        return runner([ref_slot], [list(src_slots)], composed if composed is not None else projs, depth_min, depth_max)


# -------------------------------------------------------------------------------------------------------------------------
# driver: eval.py --dataset folder --feature_cache N
# -------------------------------------------------------------------------------------------------------------------------
def _map_views(dataset, idx: int):
    scan, ref, srcs = dataset.metas[idx]
    return scan, [ref] + list(srcs[:dataset.nviews - 1])


class _Decoder:
    """host thread: per planned step, decode the images to compute (once per computation) and read the cameras of the map's
    views; items go through a bounded queue so decoding runs ahead of the GPU"""

    def __init__(self, dataset, indices, steps, dev, depth: int = 2):
        dev = torch.device(dev)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.dataset, self.indices, self.steps, self.dev = dataset, indices, steps, dev
        self.q: "queue.Queue" = queue.Queue(maxsize=max(1, depth))
        self._stop = threading.Event()
        self._cams: Dict[Key, tuple] = {}
        self.thread = threading.Thread(target=self._work, daemon=True)
        self.thread.start()

    def _put(self, item) -> bool:
        while not self._stop.is_set():
            try:
                self.q.put(item, timeout=0.1)
                return True
            except queue.Full:
                continue
        return False

    def _cam(self, scan: str, vid: int, size=None):
        from PIL import Image
        from .scan_dataset import read_cam_file
        key = (scan, vid)
        c = self._cams.get(key)
        if c is None:
            if size is None:
                with Image.open(self.dataset.image_path(scan, vid)) as im:
                    size = im.size
            k, e, dmin, dmax = read_cam_file(os.path.join(self.dataset.datapath, scan, "cams_1", "{:0>8}_cam.txt".format(vid)))
            c = self._cams[key] = (k, e, dmin, dmax, size)
        return c

    def _work(self) -> None:
        from PIL import Image
        from .scan_dataset import build_proj_matrices
        try:
            torch.cuda.set_device(self.dev)
            for idx, step in zip(self.indices, self.steps):
                scan, views = _map_views(self.dataset, idx)
                raws = []
                for (sc, vid), _ in step.compute:
                    with Image.open(self.dataset.image_path(sc, vid)) as im:
                        raw = np.asarray(im.convert("RGB"), dtype=np.uint8)
                    self._cam(sc, vid, (raw.shape[1], raw.shape[0]))
                    raws.append(raw)
                projs = {f"level_{l}": [] for l in range(4)}
                for vid in views:
                    k, e, _, _, size = self._cam(scan, vid)
                    pm = build_proj_matrices(k, e, self.dataset.img_wh, size)
                    for l in projs:
                        projs[l].append(pm[l])
                _, _, dmin, dmax, _ = self._cam(scan, views[0])
                raw = torch.from_numpy(np.stack(raws)).pin_memory() if raws else None
                item = {"raw": raw, "proj_matrices": {l: torch.from_numpy(np.stack(v)) for l, v in projs.items()},
                        "depth_min": torch.tensor(dmin, dtype=torch.float32), "depth_max": torch.tensor(dmax, dtype=torch.float32),
                        "filename": scan + "/{}/" + "{:0>8}".format(views[0]) + "{}"}
                if not self._put(item):
                    return
        except Exception as e:  # noqa: BLE001  (surfaced to the consumer)
            self._put(e)
            return
        self._put(None)

    def __iter__(self):
        try:
            while True:
                it = self.q.get()
                if it is None:
                    return
                if isinstance(it, Exception):
                    raise it
                yield it
        finally:
            self._stop.set()
            while True:
                try:
                    self.q.get_nowait()
                except queue.Empty:
                    break
            self.thread.join(timeout=5)


def save_depth_cached(args, dataset, mine: Sequence[int], model, dev, cache: ScanFeatureCache = None, write=None) -> int:
    """eval.py's folder loop (save_depth_folder) in scan mode: same PFM names, ``Iter`` lines and deferred NaN check; every
    image of the shard runs through FeatureNet once while it stays cached (``--feature_cache`` slots).  A depth map
    without source views takes the uncached path (same result or error as without the cache)."""
    from . import ops
    from .data_io import save_pfm
    from .scan_dataset import to_device
    cap = int(args.feature_cache)
    w, h = dataset.img_wh
    maps = []
    for i in mine:
        scan, views = _map_views(dataset, i)
        maps.append([(scan, v) for v in views])
    steps = plan_schedule(maps, cap, dataset.nviews)
    cache = cache if cache is not None else ScanFeatureCache(model, cap)
    model.check_nan = False
    host = [None, None]
    events = [torch.cuda.Event(), torch.cuda.Event()]
    done = 0

    def finish(job) -> None:
        name, k, n, t0 = job
        events[k].synchronize()
        depth, conf, flag = host[k]
        if int(flag[0]) != 0:
            raise AssertionError("nan in proj (singular or non-finite camera matrix, module.py:83,87)")
        print("Iter {}/{}, time = {:.3f}".format(n, len(mine), time.time() - t0))
        save_pfm(os.path.join(args.outdir, name.format("depth_est", ".pfm")), np.squeeze(depth.numpy()[0], 0))
        save_pfm(os.path.join(args.outdir, name.format("confidence", ".pfm")), np.squeeze(conf.numpy()[0], 0))

    with torch.no_grad():
        prev = None
        for n, (idx, step, item) in enumerate(zip(mine, steps, _Decoder(dataset, mine, steps, dev))):
            t0 = time.time()
            if len(step.views) == 1:                   # no source view: exactly the uncached forward (its result or its error)
                s = dataset[idx]
                imgs, projs, dmin, dmax = to_device(s, dev)
                if model.projection == "host_fp32":
                    projs = {key: v.unsqueeze(0) for key, v in s["proj_matrices"].items()}
                out = model(imgs, projs, dmin, dmax)
                d, c = out["depths_upsampled"], out["confidence_upsampled"]
            else:
                eng, slab = cache.bind(h, w)
                if step.compute:
                    raw = item["raw"].to(dev, non_blocking=True)
                    x = ops.image_pyramid(raw, h, w, all_levels=False)["level_0"]
                    cache.fill(step.compute, x)
                pm = {l: item["proj_matrices"][f"level_{l}"].float().unsqueeze(0) for l in (1, 2, 3)}
                dmin = item["depth_min"].view(1).to(dev, non_blocking=True)
                dmax = item["depth_max"].view(1).to(dev, non_blocking=True)
                composed = None
                if model.projection == "host_fp32":
                    composed = eng.compose_host(torch.stack([pm[1], pm[2], pm[3]]))
                    assert not bool(torch.isnan(composed).any()), "nan in proj (singular or non-finite camera matrix, module.py:83,87)"
                    projs = None
                else:
                    projs = {l: t.to(dev, non_blocking=True) for l, t in pm.items()}
                d, c = cache.match(step.slots[0], step.slots[1:], projs, dmin, dmax, composed=composed)
            k = n % 2
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
            prev = (item["filename"], k, n, t0)
        if prev is not None:
            finish(prev)
            done += 1
    return done
