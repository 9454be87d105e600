"""The captured cfg-4 training step (B = 4, 5 views, 640x512, bf16 features, --regress) fed by
train_dataset.TrainPrefetcher from a generated DTU tree on local disk (page cache warmed first): decode threads, pinned
batches, upload and the two input kernels on a side stream.  One JSON line: ms per fed step.  The yardstick is
tools/train_bench.py --batch 4 --graph --regress --feature_dtype bf16 (the same step with its batch already on the device).

    python tools/train_input_bench.py [--steps 20] [--warmup 5] [--num_workers 4] [--root DIR] [--phases]

The JSON line also splits the consumer's host time per timed step: ``wait_ms`` (blocked in the prefetcher's ``__next__``:
waiting for a decoded batch and for its upload event) and ``step_host_ms`` (inside ``CapturedTrainStep.step``: the copies
into the static buffers and the graph launch).  ``--phases`` then times the stages of one batch on their own, on the same
tree, in a second JSON line: decode at 1 and ``num_workers`` threads, ``collate(pin=True)``, the host-to-device copies
(device events around the uploads alone) and the two input launches (device events around them, inputs resident).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from itermvs_amd import dataset_trees, ops  # noqa: E402
from itermvs_amd.net import Pipeline  # noqa: E402
from itermvs_amd.train_dataset import DTUDataset, TrainPrefetcher, collate, epoch_batches  # noqa: E402
from itermvs_amd.train_step import CapturedTrainStep  # noqa: E402


def phases(ds, batches, dev, num_workers: int) -> dict:
    """the stages of one batch, each on its own (nothing else running), ms per batch"""
    from concurrent.futures import ThreadPoolExecutor
    res = {"metric": "training input phases per batch (ms)"}
    t = time.perf_counter()
    for b in batches[:3]:
        [ds.item(i, 0) for i in b]
    res["decode_1_thread"] = (time.perf_counter() - t) * 1e3 / 3
    with ThreadPoolExecutor(num_workers) as pool:
        t = time.perf_counter()
        for b in batches:
            list(pool.map(lambda i: ds.item(i, 0), b))
        res[f"decode_{num_workers}_threads"] = (time.perf_counter() - t) * 1e3 / len(batches)
    items = [ds.item(i, 0) for i in batches[0]]
    t = time.perf_counter()
    for _ in range(5):
        hb = collate(items, pin=True)
    res["collate_pin"] = (time.perf_counter() - t) * 1e3 / 5
    host = [hb["raw"], hb["jitter"], hb["depth_rows"], hb["mask_src"], hb["gt_params"], hb["depth_min"], hb["depth_max"]] + \
        list(hb["proj_matrices"].values())
    res["h2d_bytes"] = sum(x.numel() * x.element_size() for x in host)
    w, h = ds.img_wh
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    up_ms, k_ms = [], []
    for rep in range(13):
        ev[0].record()
        d = [x.to(dev, non_blocking=True) for x in host]
        ev[1].record()
        ops.image_pyramid_jitter(d[0], h, w, d[1])
        ops.gt_pyramid(d[2], d[3], d[4], h, w, ds.recipe)
        ev[2].record()
        torch.cuda.synchronize(dev)
        if rep >= 3:
            up_ms.append(ev[0].elapsed_time(ev[1]))
            k_ms.append(ev[1].elapsed_time(ev[2]))
    res["h2d"] = sorted(up_ms)[len(up_ms) // 2]
    res["h2d_GB_per_s"] = res["h2d_bytes"] / res["h2d"] / 1e6
    res["input_kernels"] = sorted(k_ms)[len(k_ms) // 2]
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5, help="steps before timing (>= 4: three eager steps and the capture)")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--num_workers", type=int, default=4)
    ap.add_argument("--root", default=None, help="an existing DTU tree (scan1, 15 views); generated in a temporary directory if absent")
    ap.add_argument("--resident", action="store_true", help="load every batch to the device first, then time the same steps on them "
                    "in the same order with no loader running: the step's own time on this tree's data, to compare with the fed time")
    ap.add_argument("--phases", action="store_true", help="also time decode, collate, H2D and the input kernels separately")
    args = ap.parse_args()
    tmp = None
    root = args.root
    n_views = 15
    if root is None or not os.path.isdir(os.path.join(root, "Cameras_1")):
        tmp = tempfile.TemporaryDirectory()
        root = root or tmp.name
        t = time.perf_counter()
        dataset_trees.write_dtu_tree(root, scans=("scan1",), n_views=n_views, n_src=10)
        print(f"tree written in {time.perf_counter() - t:.1f} s", file=sys.stderr)
    for dirpath, _, files in os.walk(root):                        # warm the page cache
        for f in files:
            with open(os.path.join(dirpath, f), "rb") as fh:
                while fh.read(1 << 22):
                    pass
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    model = Pipeline(iteration=4, test=False).to(dev)
    model.feature_dtype = "bf16"
    opt = torch.optim.Adam(model.parameters(), lr=torch.tensor(1e-3, device=dev), betas=(0.9, 0.999), capturable=True)
    cap = CapturedTrainStep(model, opt, True, clip=2.0)
    ds = DTUDataset(root, ["scan1"], "train", 5)
    total = args.warmup + args.steps
    batches = epoch_batches(len(ds), args.batch, 1, 0, 1, 0, max_steps=total)
    assert len(batches) == total, f"the tree holds {len(ds)} samples: {len(batches)} batches of {args.batch}"
    t0 = None
    wait, host = [], []
    pf = TrainPrefetcher(ds, batches, dev, num_workers=args.num_workers)
    it = iter(pf)
    if args.resident:
        loaded = [b for _, b in it]
        torch.cuda.synchronize(dev)
        it = iter([(None, b) for b in loaded])
    for i in range(total):
        if i == args.warmup:
            torch.cuda.synchronize(dev)
            staged0, t0 = pf.staged_ahead, time.perf_counter()
        ta = time.perf_counter()
        _, batch = next(it)
        tb = time.perf_counter()
        loss, _ = cap.step(batch)
        tc = time.perf_counter()
        if i >= args.warmup:
            wait.append((tb - ta) * 1e3)
            host.append((tc - tb) * 1e3)
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    next(it, None)                                                 # ends the iteration: the decoder thread stops
    cap.check()
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    metric = "training step on preloaded DTU-tree batches (cfg 4)" if args.resident else "fed training step (cfg 4, DTU tree, TrainPrefetcher)"
    print(json.dumps({"metric": metric, "ms_per_step": ms,
                      "samples_per_s": args.batch * 1e3 / ms, "batch": args.batch, "steps": args.steps, "warmup": args.warmup,
                      "num_workers": args.num_workers, "staged_ahead": pf.staged_ahead - staged0,
                      "wait_ms_median": med(wait), "wait_ms_mean": sum(wait) / len(wait),
                      "step_host_ms_median": med(host), "step_host_ms_mean": sum(host) / len(host), "loss": float(loss)}))
    if args.phases:
        print(json.dumps(phases(ds, batches, dev, args.num_workers)))
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
