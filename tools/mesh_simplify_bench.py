#!/usr/bin/env python3
"""The mesh simplifier (fusion.simplify_mesh: torch sorts + itermvs_mesh_simplify_*) on the sphere meshes of tools/mesh_bench.py: the
synthetic 49-view scan integrated into a cube of R^3 voxels and extracted.

    python tools/mesh_simplify_bench.py --out profiles/mesh_simplify [--shape 640x512] [--volumes 256 512] [--cells 1.5 2 4]

Per volume and cell side F (in voxels): the time of fusion.simplify_clusters (keys, the three stable sorts and the launches between
them), of the same steps with the sorts alone (keys and sort inputs exist), of the three new launches one by one into buffers that
exist, and of the whole fusion.simplify_mesh with its two read-backs; HIP events, median of --rounds after a warm-up call, rounds in
the JSON; the triangle and vertex counts before and after.  For the first volume the numpy restatement
(tests/mesh_simplify_reference.py) of the downloaded mesh on the CPU, host clock, once per cell: the only baseline there is; its
mesh must equal the GPU's.  Writes <out>/mesh_simplify_bench_<shape>.json."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mesh_bench  # noqa: E402
from itermvs_amd import fusion, ops  # noqa: E402


def sphere_mesh(h, w, res, dev):
    views = list(mesh_bench.scan(h, w, dev))
    half = mesh_bench.HALF
    plan = fusion.mesh_plan((-half,) * 3 + (half,) * 3, resolution=res, trunc_voxels=3.0, widen=False)
    state = ops.tsdf_volume(plan["dims"], dev)
    for lo in range(0, mesh_bench.N_IMG, fusion.MESH_INTEGRATE_BATCH):
        ops.tsdf_integrate(state, plan["dims"], plan["origin"], plan["voxel"], plan["trunc"], *(t[lo:lo + fusion.MESH_INTEGRATE_BATCH] for t in views))
    vertices, faces = fusion.extract_mesh(state, plan, 2)
    return vertices, faces, plan["voxel"]


def one_config(vertices, faces, voxel, factor, a, cpu):
    rec, dev = ops.MESH_VERTEX_BYTES, faces.device
    nv, nf = vertices.numel() // rec, faces.numel() // 3
    cell = factor * voxel
    xyz = vertices.view(nv, rec)[:, :12].contiguous().view(torch.float32)
    grid = fusion.simplify_grid(xyz, cell)
    out = {"cell_voxels": factor, "cell": cell, "vertices": nv, "faces": nf}
    box, info = {}, {}

    def whole():
        box["mesh"] = fusion.simplify_mesh(vertices, faces, cell, info=info)

    out["simplify_mesh_ms"], out["simplify_mesh_ms_rounds"] = mesh_bench.timed(whole, a.rounds)
    out["before_emit_ms"], out["before_emit_ms_rounds"] = mesh_bench.timed(
        lambda: box.update(parts=fusion.simplify_clusters(vertices, faces, rec, xyz, grid)), a.rounds)
    reps, cluster, hi, lo, order, _ = box["parts"]
    # the torch sorts alone, on inputs that exist
    none = torch.iinfo(torch.int64).max
    keys = ops.cloud_cell_keys(xyz, grid)
    pair, key_hi, key_lo = ops.mesh_simplify_corners(faces, cluster)

    def sorts():
        keys_sorted, perm = torch.sort(keys, stable=True)
        box["vertex_sort"] = (keys_sorted, perm)
        pair_sorted, pair_order = torch.sort(pair, stable=True)
        box["pair_sort"] = (pair_sorted, torch.div(pair_order, 3, rounding_mode="floor").to(torch.int32))
        by_lo = torch.sort(key_lo, stable=True).indices
        box["triple_sort"] = torch.sort(key_hi[by_lo], stable=True)

    out["sorts_ms"], out["sorts_ms_rounds"] = mesh_bench.timed(sorts, a.rounds)
    keys_sorted, perm = box["vertex_sort"]
    pair_sorted, pair_face = box["pair_sort"]
    cluster_sorted = torch.where(keys_sorted != none, torch.cumsum(ops.cloud_voxel_heads(keys_sorted), 0) - 1, -1).to(torch.int32)
    out["corners_ms"], out["corners_ms_rounds"] = mesh_bench.timed(lambda: ops.mesh_simplify_corners(faces, cluster), a.rounds)
    out["clusters_ms"], out["clusters_ms_rounds"] = mesh_bench.timed(
        lambda: ops.mesh_simplify_clusters(vertices, rec, faces, keys_sorted, perm, cluster_sorted, pair_sorted, pair_face, grid, reps), a.rounds)
    out_v, out_f = (torch.empty_like(t) for t in box["mesh"])
    totals = torch.zeros(2, device=dev, dtype=torch.int64)
    workspace = torch.empty(ops.mesh_simplify_emit_workspace_bytes(nv, nf), device=dev, dtype=torch.uint8)
    out["emit_ms"], out["emit_ms_rounds"] = mesh_bench.timed(
        lambda: ops.mesh_simplify_emit(reps, rec, faces, cluster, hi, lo, order, out_v, out_f, totals, workspace), a.rounds)
    assert torch.equal(out_v, box["mesh"][0]) and torch.equal(out_f, box["mesh"][1])
    out.update({k: info[k] for k in ("clusters", "valid_faces", "degenerate_faces", "duplicate_faces", "simplify_bytes")},
               vertices_after=info["vertices"], faces_after=info["faces"])
    if cpu:
        import mesh_simplify_reference as S
        host_v, host_f = vertices.cpu().numpy().reshape(-1, rec), faces.cpu().numpy().reshape(-1, 3)
        t0 = time.perf_counter()
        want_v, want_f, _ = S.simplify(host_v, host_f, cell)
        out["cpu_restatement_ms"] = 1e3 * (time.perf_counter() - t0)
        out["cpu_equals_gpu"] = bool(want_v.tobytes() == out_v.cpu().numpy().tobytes() and want_f.tobytes() == out_f.cpu().numpy().tobytes())
        assert out["cpu_equals_gpu"]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="profiles/mesh_simplify")
    p.add_argument("--shape", default="640x512")
    p.add_argument("--volumes", nargs="+", type=int, default=[256, 512])
    p.add_argument("--cells", nargs="+", type=float, default=[1.5, 2.0, 4.0])
    p.add_argument("--rounds", type=int, default=5)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_simplify_bench.py measures on the GPU: none found")
    dev = torch.device("cuda")
    os.makedirs(a.out, exist_ok=True)
    w, h = (int(s) for s in a.shape.split("x"))
    results = []
    for n, res in enumerate(a.volumes):
        vertices, faces, voxel = sphere_mesh(h, w, res, dev)
        for factor in a.cells:
            r = dict(shape=f"{w}x{h}", volume=res, **one_config(vertices, faces, voxel, factor, a, cpu=n == 0))
            results.append(r)
            print(json.dumps({k: v for k, v in r.items() if not k.endswith("_rounds")}), flush=True)
    with open(os.path.join(a.out, f"mesh_simplify_bench_{a.shape}.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
