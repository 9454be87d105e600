#!/usr/bin/env python3
"""The two stages of eval.py --mesh on one synthetic 49-view scan: a sphere of radius 150 at the origin seen by the rig of
itermvs_amd.synthetic (analytic depth maps, every pixel unmasked), integrated into a cube of R^3 voxels around it and extracted.

    python tools/mesh_bench.py --out profiles/mesh [--shapes 640x512 1600x1152] [--volumes 256 512] [--batches 1 2 4 7 16 49]

Per (shape, volume) and batch size: the time of integrating the 49 views (HIP events around the launches, median of --rounds after
a warm-up pass), the bytes of volume state the launches move (12 read + 12 written per voxel and LAUNCH) per second, and next to it
the rate of a device-to-device copy of the same state buffer (12 read + 12 written per voxel) measured in the same process.  Their
ratio says how close the batched kernel is to the traffic it cannot avoid.  Extraction: the time of fusion.extract_mesh (its two
runs of itermvs_tsdf_mesh and the allocation between them) and of one itermvs_tsdf_mesh into buffers that exist.  Writes
<out>/mesh_bench_<shape>.json."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from itermvs_amd import fusion, ops, synthetic  # noqa: E402

N_IMG, RADIUS, HALF = 49, 150.0, 200.0


def scan(h, w, dev):
    """-> depth float64 [49,h,w], mask uint8, cams float32 [49,21], rgb uint8 on the GPU"""
    k0, exts = synthetic.camera_parameters(N_IMG, h, w)
    y, x = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float64), torch.arange(w, device=dev, dtype=torch.float64), indexing="ij")
    ray = torch.stack([(x - k0[0, 2]) / k0[0, 0], (y - k0[1, 2]) / k0[1, 1], torch.ones_like(x)], -1)
    depth = torch.empty((N_IMG, h, w), device=dev, dtype=torch.float64)
    for v, e in enumerate(exts):
        r = torch.from_numpy(np.asarray(e, np.float64)[:3, :3]).to(dev)
        c = -(r.T @ torch.from_numpy(np.asarray(e, np.float64)[:3, 3]).to(dev))
        d = ray @ r
        a, b, cc = (d * d).sum(-1), 2 * (d @ c), c @ c - RADIUS ** 2
        disc = b * b - 4 * a * cc
        depth[v] = torch.where(disc > 0, (-b - torch.sqrt(disc.clamp(min=0))) / (2 * a), torch.zeros_like(a))
    cams = np.stack([np.concatenate([k0.reshape(-1), np.asarray(e, np.float64)[:3].reshape(-1)]) for e in exts]).astype(np.float32)
    rgb = torch.randint(0, 256, (N_IMG, h, w, 3), device=dev, dtype=torch.uint8, generator=torch.Generator(dev).manual_seed(0))
    return depth, torch.ones((N_IMG, h, w), device=dev, dtype=torch.uint8), torch.from_numpy(cams).to(dev), rgb


def timed(fn, rounds):
    """median milliseconds of ``fn`` between two events, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def one_config(h, w, res, batches, rounds, dev):
    views = scan(h, w, dev)
    plan = fusion.mesh_plan((-HALF,) * 3 + (HALF,) * 3, resolution=res, trunc_voxels=3.0, widen=False)
    n = res ** 3
    state = ops.tsdf_volume(plan["dims"], dev)
    other = torch.empty_like(state)
    copy_ms, _ = timed(lambda: other.copy_(state), rounds)
    del other
    out = {"shape": f"{w}x{h}", "volume": res, "voxels": n, "state_bytes": plan["state_bytes"], "copy_ms": copy_ms,
           "copy_gb_per_s": 24 * n / copy_ms / 1e6, "integrate": []}

    def integrate(batch):
        state.zero_()
        for a in range(0, N_IMG, batch):
            ops.tsdf_integrate(state, plan["dims"], plan["origin"], plan["voxel"], plan["trunc"], *(t[a:a + batch] for t in views))

    zero_ms, _ = timed(state.zero_, rounds)
    for batch in batches:
        ms, all_ms = timed(lambda: integrate(batch), rounds)
        ms -= zero_ms                                              # the reset of the volume is not part of the stage
        launches = (N_IMG + batch - 1) // batch
        out["integrate"].append({"batch": batch, "launches": launches, "ms": ms, "ms_rounds": [m - zero_ms for m in all_ms],
                                 "state_gb_per_s": 24 * n * launches / ms / 1e6,
                                 "share_of_copy_rate": (24 * n * launches / ms) / (24 * n / copy_ms)})
    integrate(batches[-1])
    box = {}

    def extract():
        box["mesh"] = fusion.extract_mesh(state, plan, 2)

    out["extract_ms"], _ = timed(extract, rounds)
    vertices, faces = box["mesh"]
    totals = torch.zeros(2, device=dev, dtype=torch.int64)
    workspace = torch.empty(ops.tsdf_mesh_workspace_bytes(plan["dims"]), device=dev, dtype=torch.uint8)
    out["mesh_call_ms"], _ = timed(lambda: ops.tsdf_mesh(state, plan["dims"], plan["origin"], plan["voxel"], 2, vertices, faces, totals,
                                                         workspace), rounds)
    out.update(vertices=vertices.numel() // ops.MESH_VERTEX_BYTES, faces=faces.numel() // 3, zero_ms=zero_ms)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="profiles/mesh")
    p.add_argument("--shapes", nargs="+", default=["640x512", "1600x1152"])
    p.add_argument("--volumes", nargs="+", type=int, default=[256, 512])
    p.add_argument("--batches", nargs="+", type=int, default=[1, 2, 4, 7, 16, 49])
    p.add_argument("--rounds", type=int, default=5)
    a = p.parse_args()
    dev = torch.device("cuda")
    os.makedirs(a.out, exist_ok=True)
    for shape in a.shapes:
        w, h = (int(s) for s in shape.split("x"))
        results = [one_config(h, w, res, a.batches, a.rounds, dev) for res in a.volumes]
        with open(os.path.join(a.out, f"mesh_bench_{shape}.json"), "w") as f:
            json.dump(results, f, indent=1)
        for r in results:
            print(json.dumps({k: v for k, v in r.items() if k != "integrate"}))
            for row in r["integrate"]:
                print("   ", json.dumps({k: v for k, v in row.items() if k != "ms_rounds"}))


if __name__ == "__main__":
    main()
