#!/usr/bin/env python3
"""Scan mode against the per-sample path on one synthetic 49-view scan (DTU-like pair lists: every view is the reference
once with its 10 neighbours listed, n_views 5 -> the first 4 are read).  In one process, alternating: the uncached
captured-graph path (Pipeline.forward, FeatureNet on all 5 views of every depth map) and the cached path
(itermvs_amd.scan_cache: each image's pyramid once, CachedRunner per depth map).  The images are already on the GPU for
both paths (no decode / upload is timed), so the figures are the GPU work of the two paths.

    python tools/scan_bench.py --out profiles/scan_bench [--shapes 640x512 1600x1152] [--dtypes fp32 fp16] [--rounds 3]

Writes <out>/scan_bench.json: per (shape, feature dtype) depth maps/s of both paths (median of the rounds), FeatureNet
images per depth map, the slab's HBM footprint, the time to stage one reference view's maps, and whether every depth and
confidence map of the cached path equals the uncached one bit for bit."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from itermvs_amd import ops, synthetic  # noqa: E402
from itermvs_amd.net import Pipeline  # noqa: E402
from itermvs_amd.scan_cache import ScanFeatureCache, plan_schedule  # noqa: E402

N_IMG, N_VIEWS, NEIGHBOURS = 49, 5, 10


def pair_lists(n=N_IMG):
    out = []
    for r in range(n):
        nb = []
        for k in range(1, NEIGHBOURS // 2 + 1):
            nb += [(r + k) % n, (r - k) % n]
        out.append((r, nb))
    return out


def one_config(h, w, dtype, rounds, iteration, only=None):
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    imgs = (torch.rand(N_IMG, 3, h, w, generator=gen) * 2 - 1).to(dev)
    cams = synthetic.make_cameras(N_IMG, h, w)
    pm = {l: torch.from_numpy(cams[f"level_{l}"]).to(dev) for l in (1, 2, 3)}
    maps = [[r] + nb[:N_VIEWS - 1] for r, nb in pair_lists()]
    dmin, dmax = torch.tensor([425.0], device=dev), torch.tensor([935.0], device=dev)
    model = Pipeline(iteration=iteration, test=True)
    model.load_state_dict(synthetic.random_state_dict(0))
    model.feature_dtype, model.use_graphs, model.check_nan = dtype, True, False
    model = model.to(dev).eval()
    projs = [{f"level_{l}": pm[l][m].unsqueeze(0).contiguous() for l in (1, 2, 3)} for m in maps]
    projs_l = [{l: p[f"level_{l}"] for l in (1, 2, 3)} for p in projs]
    x_maps = [imgs[m].unsqueeze(0).contiguous() for m in maps]
    want = []

    def uncached(keep):
        for i in range(N_IMG):
            out = model({"level_0": x_maps[i]}, projs[i], dmin, dmax)
            if keep:
                want.append((out["depths_upsampled"].clone(), out["confidence_upsampled"].clone()))

    cache = ScanFeatureCache(model, N_IMG)
    same = [True]

    def cached(check):
        steps = plan_schedule(maps, N_IMG, N_VIEWS)
        cache.computed = 0
        for i, st in enumerate(steps):
            cache.bind(h, w)
            if st.compute:
                cache.fill(st.compute, imgs[[k for k, _ in st.compute]])
            d, c = cache.match(st.slots[0], st.slots[1:], projs_l[i], dmin, dmax)
            if check:
                same[0] = same[0] and torch.equal(d, want[i][0]) and torch.equal(c, want[i][1])

    if only is not None:        # one path alone (a profiler run of that path): warm-up, then the rounds
        fn = uncached if only == "uncached" else cached
        with torch.no_grad():
            fn(False)
            torch.cuda.synchronize()
            t = []
            for _ in range(rounds):
                t0 = time.perf_counter()
                fn(False)
                torch.cuda.synchronize()
                t.append(time.perf_counter() - t0)
        return {"shape": f"{w}x{h}", "feature_dtype": dtype, "path": only, "maps_per_s": N_IMG / statistics.median(t), "round_s": t}
    with torch.no_grad():
        uncached(True)          # warm-up: captures the graph, keeps the reference outputs
        cached(True)            # warm-up: captures the matching graph, checks every map
        torch.cuda.synchronize()
        t_unc, t_cac = [], []
        for _ in range(rounds):
            for fn, acc in ((uncached, t_unc), (cached, t_cac)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(False)
                torch.cuda.synchronize()
                acc.append(time.perf_counter() - t0)
        cached(True)
        torch.cuda.synchronize()
        model.check_projection_finite()
        # staging of one reference view's maps (the part of CachedRunner.__call__ that copies from the slab)
        runner = next(iter(cache.runners.values()))
        slab = cache.slab
        flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1)
        dst = [flat(runner.ref[l]) for l in (1, 2, 3)] + [runner.ref2.reshape(-1)]
        src = [flat(slab.levels[l][7:8]) for l in (1, 2, 3)] + [slab.planar[7:8].reshape(-1)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            ops.copy_multi(dst, src)
        e0.record()
        for _ in range(20):
            ops.copy_multi(dst, src)
        e1.record()
        torch.cuda.synchronize()
        stage_us = e0.elapsed_time(e1) / 20 * 1000
    mu, mc = statistics.median(t_unc), statistics.median(t_cac)
    return {"shape": f"{w}x{h}", "feature_dtype": dtype, "iteration": iteration, "depth_maps": N_IMG, "rounds": rounds,
            "uncached_maps_per_s": N_IMG / mu, "cached_maps_per_s": N_IMG / mc, "speedup": mu / mc,
            "uncached_round_s": t_unc, "cached_round_s": t_cac,
            "featurenet_images_per_map_uncached": float(N_VIEWS), "featurenet_images_per_map_cached": cache.computed / N_IMG,
            "cache_bytes": cache.slab.nbytes, "cache_bytes_per_image": cache.slab.nbytes // N_IMG,
            "ref_staging_us": stage_us, "bit_identical": bool(same[0])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--shapes", nargs="+", default=["640x512", "1600x1152"])
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "fp16"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iteration", type=int, default=4)
    ap.add_argument("--only", choices=["uncached", "cached"], help="time one path alone (for a profiler run)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "results": []}
    for shp in a.shapes:
        w, h = (int(v) for v in shp.split("x"))
        for dt in a.dtypes:
            r = one_config(h, w, dt, a.rounds, a.iteration, a.only)
            print(json.dumps(r), flush=True)
            res["results"].append(r)
            torch.cuda.empty_cache()
    with open(os.path.join(a.out, "scan_bench.json" if a.only is None else f"scan_bench_{a.only}.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
