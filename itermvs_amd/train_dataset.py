"""Training datasets (reference: datasets/dtu_yao.py, datasets/blendedmvs.py) with a GPU training input side.

``DTUDataset`` ('dtu_yao') and ``BlendedMVSDataset`` ('blendedmvs') read the reference's on-disk layouts and follow its
``__getitem__`` semantics, but an item holds only the host-side part of the sample: the decoded uint8 RGB views, the raw
PFM payload of the reference view (rows bottom-up, as stored), DTU's ``depth_visual`` bytes, the projection matrices,
``depth_min`` / ``depth_max`` and one ColorJitter draw per view.  ``to_device`` turns a collated batch into the reference's
collated training sample on the GPU -- (imgs, proj_matrices, depth_min, depth_max, depth, mask), the 6-tuple
``train.train_step`` and ``train_step.CapturedTrainStep`` take -- with two HIP launches per batch: the jittered image
pyramid (``itermvs_image_pyramid_jitter``) and the ground-truth pyramids (``itermvs_gt_pyramid``).  ``TrainPrefetcher``
decodes the next batches on a small thread pool and stages one batch ahead on a side stream, like
``scan_dataset.Prefetcher``.

ColorJitter: torchvision's ``ColorJitter(brightness=0.5, contrast=0.5).get_params`` draws ``randperm(4)``, then the
brightness factor ``uniform_(0.5, 1.5)``, then the contrast factor ``uniform_(0.5, 1.5)`` (saturation and hue are None and
draw nothing); ``forward`` applies brightness before contrast iff index 0 precedes index 1 in the permutation, each as
``PIL.ImageEnhance`` computes it.  torchvision is not a dependency: the sequence is written here from its documented
behaviour.  ``depth_min`` / ``depth_max`` reach the device as float32 (the engine's type; the reference's collate makes
float64 tensors of the same Python floats).

Deliberate deviations from the reference:
- Random draws come from a per-sample generator seeded by (seed, epoch, sample index): a ``random.Random`` for the source
  view subset and the depth scale, a ``torch.Generator`` for the jitter -- not from the process-global RNGs.  Batches are
  then independent of decode-thread scheduling; the reference's global draws under 4 worker processes are not reproducible
  anyway.
- BlendedMVS scale factor: the reference sets ``scale_factors[scan] = 100 / depth_min`` from whichever camera file of the
  scan its process reads first (blendedmvs.py:55-56), which depends on read order.  Here it is fixed when the dataset is
  built: 100 / depth_min of the scan's first reference view in ``pair.txt``.
"""
from __future__ import annotations

import collections
import hashlib
import os
import random
import re
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .scan_dataset import Prefetcher

JITTER_DTYPE = np.dtype([("brightness", "<f4"), ("contrast", "<f4"), ("contrast_first", "<i4"), ("enabled", "<i4")])
LIGHTS = 7                                   # dtu_yao.py:43-45


def sample_key(seed: int, epoch: int, index: int) -> int:
    """63-bit seed of one sample's generators, a function of (seed, epoch, index) only"""
    h = hashlib.sha256(f"itermvs-train/{int(seed)}/{int(epoch)}/{int(index)}".encode()).digest()
    return int.from_bytes(h[:8], "little") >> 1


def color_jitter_params(gen: torch.Generator) -> Tuple[float, float, bool]:
    """torchvision ColorJitter(brightness=0.5, contrast=0.5).get_params on ``gen`` -> (brightness, contrast,
    contrast_first): randperm(4), then uniform_(0.5, 1.5) for brightness, then for contrast"""
    perm = torch.randperm(4, generator=gen).tolist()
    b = float(torch.empty(1).uniform_(0.5, 1.5, generator=gen))
    c = float(torch.empty(1).uniform_(0.5, 1.5, generator=gen))
    return b, c, perm.index(1) < perm.index(0)


def jitter_records(draws: Sequence[Optional[Tuple[float, float, bool]]]) -> np.ndarray:
    """itermvs_jitter records (include/itermvs_hip.h) for a list of draws (None = no jitter)"""
    rec = np.zeros(len(draws), JITTER_DTYPE)
    for i, d in enumerate(draws):
        if d is None:
            rec[i] = (1.0, 1.0, 0, 0)
        else:
            rec[i] = (d[0], d[1], int(d[2]), 1)
    return rec


def read_cam_file(filename: str):
    """dtu_yao.py:52-62 / blendedmvs.py:45-54 -> (intrinsics [3,3] f32, extrinsics [4,4] f32, depth_min, depth_max)"""
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = np.fromstring(" ".join(lines[1:5]), dtype=np.float32, sep=" ").reshape((4, 4))
    intrinsics = np.fromstring(" ".join(lines[7:10]), dtype=np.float32, sep=" ").reshape((3, 3))
    return intrinsics, extrinsics, float(lines[11].split()[0]), float(lines[11].split()[-1])


def proj_levels(intrinsics: np.ndarray, extrinsics: np.ndarray) -> Dict[str, np.ndarray]:
    """the shared tail of dtu_yao.py:170-188 / blendedmvs.py:148-166: K[:2] x0.125, P = K @ E[:3,:4] for level 3, then
    three doublings for levels 2, 1, 0 (float32, in place, in that order)"""
    k = intrinsics
    out = {}
    k[:2, :] *= 0.125
    for lvl in (3, 2, 1, 0):
        if lvl != 3:
            k[:2, :] *= 2
        p = extrinsics.copy()
        p[:3, :4] = np.matmul(k, p[:3, :4])
        out[f"level_{lvl}"] = p
    return out


def read_pfm_rows(filename: str) -> np.ndarray:
    """a 1-channel PFM's payload as stored (rows bottom-up) as native float32 [H,W] -- data_io.py:6-42 without the flip,
    which itermvs_gt_pyramid absorbs into its index map"""
    with open(filename, "rb") as f:
        if f.readline().rstrip() != b"Pf":
            raise ValueError(f"{filename}: expected a 1-channel PFM ('Pf')")
        m = re.match(rb"^(\d+)\s(\d+)\s$", f.readline())
        if not m:
            raise ValueError(f"{filename}: malformed PFM header")
        w, h = int(m.group(1)), int(m.group(2))
        scale = float(f.readline().rstrip())
        data = np.fromfile(f, ("<" if scale < 0 else ">") + "f4", count=w * h)
    if data.size != w * h:
        raise ValueError(f"{filename}: truncated PFM")
    return data.astype(np.float32, copy=False).reshape(h, w)


def read_rgb(filename: str) -> np.ndarray:
    from PIL import Image
    with Image.open(filename) as im:
        if im.mode != "RGB":
            im = im.convert("RGB")
        return np.asarray(im, dtype=np.uint8)


def read_pair_list(filename: str) -> List[Tuple[int, List[int]]]:
    with open(filename) as f:
        n = int(f.readline())
        out = []
        for _ in range(n):
            ref = int(f.readline().rstrip())
            out.append((ref, [int(x) for x in f.readline().rstrip().split()[1::2]]))
    return out


def read_list(listfile) -> List[str]:
    if isinstance(listfile, str):
        with open(listfile) as f:
            return [line.rstrip() for line in f.readlines()]
    return list(listfile)


class _TrainDataset(torch.utils.data.Dataset):
    recipe = None

    def __init__(self, datapath: str, listfile, mode: str, nviews: int, img_wh: Sequence[int], seed: int):
        if mode not in ("train", "val"):
            raise ValueError("mode must be 'train' or 'val'")
        self.datapath, self.mode, self.nviews, self.img_wh, self.seed = datapath, mode, int(nviews), tuple(img_wh), int(seed)
        self.epoch = 0
        self.scans = read_list(listfile)

    def __len__(self) -> int:
        return len(self.metas)

    def draws(self, idx: int, epoch: int):
        """-> (view ids, scale, per-view jitter draws or Nones): robust_train in train mode (dtu_yao.py:126-134), the first
        nviews - 1 sources, scale 1 and no jitter in val mode"""
        ref_view, src_views = self.metas[idx][-2:]
        if self.mode != "train":
            return [ref_view] + src_views[:self.nviews - 1], 1, [None] * self.nviews
        key = sample_key(self.seed, epoch, idx)
        rnd = random.Random(key)
        index = rnd.sample(range(len(src_views)), self.nviews - 1)
        scale = rnd.uniform(0.8, 1.25)
        gen = torch.Generator().manual_seed(key)
        return [ref_view] + [src_views[i] for i in index], scale, [color_jitter_params(gen) for _ in range(self.nviews)]

    def __getitem__(self, idx: int) -> dict:
        return self.item(idx, self.epoch)

    def _sample(self, raws, projs, depth_rows, mask_src, params, depth_min, depth_max, jitter) -> dict:
        if any(r.shape != raws[0].shape for r in raws):
            raise ValueError("the views of one sample must share the image size")
        return {"raw": np.stack(raws), "proj_matrices": {l: np.stack(v) for l, v in projs.items()},
                "depth_rows": depth_rows, "mask_src": mask_src, "gt_params": np.asarray(params, np.float32),
                "depth_min": depth_min, "depth_max": depth_max, "jitter": jitter_records(jitter)}


class DTUDataset(_TrainDataset):
    """datasets/dtu_yao.py: metas = scans x Cameras_1/pair.txt views x 7 lights (:28-47), the same list for train and val"""
    recipe = _lib.GT_DTU

    def __init__(self, datapath: str, listfile, mode: str = "train", nviews: int = 5, img_wh=(640, 512), seed: int = 1):
        super().__init__(datapath, listfile, mode, nviews, img_wh, seed)
        pairs = read_pair_list(os.path.join(datapath, "Cameras_1/pair.txt"))
        self.metas = [(scan, light, ref, srcs) for scan in self.scans for ref, srcs in pairs for light in range(LIGHTS)]

    def paths(self, scan: str, light: int, vid: int) -> Dict[str, str]:
        j = lambda p: os.path.join(self.datapath, p)  # noqa: E731
        return {"image": j("Rectified/{}_train/rect_{:0>3}_{}_r5000.png".format(scan, vid + 1, light)),
                "cam": j("Cameras_1/{}_train/{:0>8}_cam.txt".format(scan, vid)),
                "depth": j("Depths_raw/{}/depth_map_{:0>4}.pfm".format(scan, vid)),
                "mask": j("Depths_raw/{}/depth_visual_{:0>4}.png".format(scan, vid))}

    def item(self, idx: int, epoch: int) -> dict:
        from PIL import Image
        scan, light, _, _ = self.metas[idx]
        view_ids, scale, jitter = self.draws(idx, epoch)
        raws, projs = [], {f"level_{l}": [] for l in range(4)}
        for i, vid in enumerate(view_ids):
            p = self.paths(scan, light, vid)
            raws.append(read_rgb(p["image"]))
            intrinsics, extrinsics, dmin, dmax = read_cam_file(p["cam"])
            extrinsics[:3, 3] *= scale                                       # dtu_yao.py:165-168
            intrinsics[0] *= 4
            intrinsics[1] *= 4
            for l, m in proj_levels(intrinsics, extrinsics).items():
                projs[l].append(m)
            if i == 0:
                depth_min, depth_max = dmin * scale, dmax * scale
                rows = read_pfm_rows(p["depth"])
                with Image.open(p["mask"]) as im:
                    mask = np.asarray(im)
                if mask.dtype != np.uint8 or mask.shape != rows.shape:
                    raise ValueError(f"{p['mask']}: expected an 8-bit single-channel image of the depth map's size")
        params = (np.float32(scale), 1.0, 0.0, 0.0)
        return self._sample(raws, projs, rows, mask, params, depth_min, depth_max, jitter)


class BlendedMVSDataset(_TrainDataset):
    """datasets/blendedmvs.py: metas keep the reference views with at least nviews - 1 sources (:32-43)"""
    recipe = _lib.GT_BLENDEDMVS

    def __init__(self, datapath: str, listfile, mode: str = "train", nviews: int = 5, img_wh=(768, 576), seed: int = 1):
        super().__init__(datapath, listfile, mode, nviews, img_wh, seed)
        if self.img_wh[0] % 32 or self.img_wh[1] % 32:
            raise ValueError("img_wh must both be multiples of 32!")
        self.metas, self.scale_factors = [], {}
        for scan in self.scans:
            pairs = read_pair_list(os.path.join(datapath, scan, "cams/pair.txt"))
            if pairs:               # fixed rule (module docstring): 100 / depth_min of the first reference view in pair.txt
                self.scale_factors[scan] = 100.0 / read_cam_file(self.paths(scan, pairs[0][0])["cam"])[2]
            self.metas += [(scan, ref, srcs) for ref, srcs in pairs if len(srcs) >= self.nviews - 1]

    def paths(self, scan: str, vid: int) -> Dict[str, str]:
        j = lambda p: os.path.join(self.datapath, p)  # noqa: E731
        return {"image": j("{}/blended_images/{:0>8}.jpg".format(scan, vid)),
                "depth": j("{}/rendered_depth_maps/{:0>8}.pfm".format(scan, vid)),
                "cam": j("{}/cams/{:0>8}_cam.txt".format(scan, vid))}

    def item(self, idx: int, epoch: int) -> dict:
        scan = self.metas[idx][0]
        sf = self.scale_factors[scan]
        view_ids, scale, jitter = self.draws(idx, epoch)
        raws, projs = [], {f"level_{l}": [] for l in range(4)}
        for i, vid in enumerate(view_ids):
            p = self.paths(scan, vid)
            raws.append(read_rgb(p["image"]))
            intrinsics, extrinsics, dmin, dmax = read_cam_file(p["cam"])
            dmin, dmax = dmin * sf, dmax * sf                                 # blendedmvs.py:57-59
            extrinsics[:3, 3] *= sf
            extrinsics[:3, 3] *= scale                                        # blendedmvs.py:147
            for l, m in proj_levels(intrinsics, extrinsics).items():
                projs[l].append(m)
            if i == 0:
                depth_min, depth_max = dmin * scale, dmax * scale
                rows = read_pfm_rows(p["depth"])
        # float32 range: numpy compares the float32 depth with the Python floats rounded to float32 (blendedmvs.py:67)
        params = (np.float32(sf), np.float32(scale), np.float32(depth_min), np.float32(depth_max))
        return self._sample(raws, projs, rows, None, params, depth_min, depth_max, jitter)


DATASETS = {"dtu_yao": DTUDataset, "blendedmvs": BlendedMVSDataset}


def _stack(arrays: Sequence[np.ndarray], pin: bool) -> torch.Tensor:
    """np.stack into a (pinned) torch tensor, the bulk copies done by torch (which releases the GIL: a multi-megabyte
    numpy copy holds it, and the training loop's thread then waits for the GIL to enqueue the next step)"""
    first = arrays[0]
    if any(a.shape != first.shape or a.dtype != first.dtype for a in arrays):
        raise ValueError("the samples of one batch must share their sizes")
    out = torch.empty((len(arrays),) + first.shape, dtype=torch.from_numpy(first.reshape(-1)[:0]).dtype, pin_memory=pin)
    for i, a in enumerate(arrays):
        out[i].copy_(torch.from_numpy(a if a.flags.c_contiguous else np.ascontiguousarray(a)))
    return out


def collate(samples: Sequence[dict], pin: bool = False) -> dict:
    """host-side batch of ``item``s (same sizes): uint8 views [B*V,Hs,Ws,3], jitter records [B*V], PFM rows [B,Hs,Ws],
    depth_visual [B,Hs,Ws] or None, gt params [B,4], projections [B,V,4,4], depth range [B] float32"""
    raw = _stack([s["raw"] for s in samples], pin)
    return {"raw": raw.view((-1,) + tuple(raw.shape[2:])), "n_views": raw.shape[1],
            "jitter": _stack([s["jitter"].view(np.uint8) for s in samples], pin).view(-1),
            "depth_rows": _stack([s["depth_rows"] for s in samples], pin),
            "mask_src": None if samples[0]["mask_src"] is None else _stack([s["mask_src"] for s in samples], pin),
            "gt_params": _stack([s["gt_params"] for s in samples], pin),
            "proj_matrices": {l: _stack([s["proj_matrices"][l] for s in samples], pin) for l in samples[0]["proj_matrices"]},
            "depth_min": _stack([np.array(s["depth_min"], np.float32) for s in samples], pin),
            "depth_max": _stack([np.array(s["depth_max"], np.float32) for s in samples], pin)}


def to_device(batch: dict, dev, img_wh: Sequence[int], recipe: int):
    """collated batch -> (imgs, proj_matrices, depth_min, depth_max, depth, mask) on ``dev``, the reference's collated
    training sample: imgs level_0..3 [B,V,3,H>>l,W>>l], depth / mask level_0..3 [B,1,H>>l,W>>l]; enqueued on the current
    stream (uploads + itermvs_image_pyramid_jitter + itermvs_gt_pyramid)"""
    from . import ops
    up = lambda x: x.to(dev, non_blocking=True)  # noqa: E731
    w, h = img_wh
    b, v = batch["depth_rows"].shape[0], batch["n_views"]
    imgs = {k: x.view((b, v) + tuple(x.shape[1:]))
            for k, x in ops.image_pyramid_jitter(up(batch["raw"]), h, w, up(batch["jitter"])).items()}
    depth, mask = ops.gt_pyramid(up(batch["depth_rows"]), None if batch["mask_src"] is None else up(batch["mask_src"]),
                                 up(batch["gt_params"]), h, w, recipe)
    projs = {k: up(x) for k, x in batch["proj_matrices"].items()}
    return imgs, projs, up(batch["depth_min"]), up(batch["depth_max"]), depth, mask


def epoch_permutation(n: int, seed: int, epoch: int) -> List[int]:
    """the epoch's shuffle, the same on every rank"""
    return torch.randperm(n, generator=torch.Generator().manual_seed(sample_key(seed, epoch, -1))).tolist()


def epoch_batches(n: int, batch: int, world: int, rank: int, seed: int, epoch: int, train: bool = True,
                  max_steps: Optional[int] = None) -> List[List[int]]:
    """this rank's batches of one epoch.  train: DataLoader(shuffle=True, drop_last=True) over all ranks (train.py:89):
    ``n // (batch * world)`` steps, step s of rank r = permutation[(s * world + r) * batch : ... + batch].  val
    (train.py:90, shuffle=False, drop_last=False): the batches of 0..n-1 in order, batch k to rank k % world"""
    if train:
        perm = epoch_permutation(n, seed, epoch)
        out = [perm[(s * world + rank) * batch:(s * world + rank + 1) * batch] for s in range(n // (batch * world))]
    else:
        out = [list(range(k, min(k + batch, n))) for k in range(0, n, batch)][rank::world]
    return out if max_steps is None else out[:max_steps]


class TrainPrefetcher(Prefetcher):
    """Iterates batches of a training dataset (lists of indices, e.g. ``epoch_batches``) as the 6-tuple on the device, in
    order: ``num_workers`` decode threads (PIL releases the GIL while decoding; never sized from the CPU count), pinned
    host batches, upload + the two kernels on a side stream, one batch staged ahead, the host waiting on the batch's event
    (no cross-stream wait) -- the mechanics of ``scan_dataset.Prefetcher``.  Yields (host batch, device 6-tuple)."""

    def __init__(self, dataset, batches: Sequence[Sequence[int]], dev, num_workers: int = 4, epoch: int = 0, depth: int = 2):
        self.num_workers, self.epoch = max(1, int(num_workers)), int(epoch)
        super().__init__(dataset, [list(b) for b in batches], dev, depth)

    def _work(self) -> None:
        try:
            torch.cuda.set_device(self.dev)
            with ThreadPoolExecutor(self.num_workers) as pool:
                pending = collections.deque()
                todo = iter(self.indices)

                def submit() -> None:
                    nxt = next(todo, None)
                    if nxt is not None:
                        pending.append([pool.submit(self.dataset.item, i, self.epoch) for i in nxt])

                for _ in range(2):                          # two batches in decode: the threads never idle at a boundary
                    submit()
                while pending:
                    futs = pending.popleft()
                    submit()
                    batch = collate([f.result() for f in futs], pin=True)
                    if not self._put(batch):
                        for fs in pending:
                            for f in fs:
                                f.cancel()
                        return
        except Exception as e:  # noqa: BLE001  (surfaced to the consumer)
            self._put(e)
            return
        self._put(None)

    def _to_device(self, s):
        return to_device(s, self.dev, self.dataset.img_wh, self.dataset.recipe)

    def _device_tensors(self, tensors):
        imgs, projs, dmin, dmax, depth, mask = tensors
        return list(imgs.values()) + list(projs.values()) + [dmin, dmax] + list(depth.values()) + list(mask.values())
