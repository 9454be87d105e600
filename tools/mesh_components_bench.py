#!/usr/bin/env python3
"""The component filter of the mesh (itermvs_mesh_components, itermvs_mesh_keep) on the synthetic 49-view scan of tools/mesh_bench.py
with floating fragments: the sphere of radius 150 plus --blobs small spheres of radius --blob_radius scattered outside it inside the
volume, all ray-cast analytically into every view, integrated into a cube of R^3 voxels and extracted.

    python tools/mesh_components_bench.py --out profiles/mesh_components [--shape 640x512] [--volumes 256 512]

Per volume: the time of fusion.extract_mesh in the same run, of one itermvs_mesh_components (memset + 5 launches, its label and
count buffers allocated), of one itermvs_mesh_keep into buffers that exist, and of fusion.keep_mesh_components (both, the three
read-backs and the allocations between them), HIP events, median of --rounds after a warm-up call, rounds in the JSON; the counts;
the bytes the download no longer carries; and the same filter on the CPU for the downloaded mesh (scipy connected_components +
a numpy compaction; host clock, median of --cpu_rounds), whose kept mesh must equal the GPU's.  Writes
<out>/mesh_components_bench_<shape>.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mesh_bench  # noqa: E402
from itermvs_amd import fusion, ops, synthetic  # noqa: E402


def add_blobs(depth, h, w, n_blobs, radius, dev):
    """the nearest of the sphere's depth and the blobs', per view, in place; blob centres: seeded, on the shell 170..185 from the
    origin (outside the sphere of 150, inside the cube of half side 200 in every direction)"""
    rng = np.random.default_rng(4)
    d = rng.normal(size=(n_blobs, 3))
    centres = torch.from_numpy(d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(170.0, 185.0, (n_blobs, 1))).to(dev)
    k0, exts = synthetic.camera_parameters(mesh_bench.N_IMG, h, w)
    y, x = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float64), torch.arange(w, device=dev, dtype=torch.float64), indexing="ij")
    ray = torch.stack([(x - k0[0, 2]) / k0[0, 0], (y - k0[1, 2]) / k0[1, 1], torch.ones_like(x)], -1)
    for v, e in enumerate(exts):
        r = torch.from_numpy(np.asarray(e, np.float64)[:3, :3]).to(dev)
        c = -(r.T @ torch.from_numpy(np.asarray(e, np.float64)[:3, 3]).to(dev))
        dirs = ray @ r
        a = (dirs * dirs).sum(-1)
        for lo in range(0, n_blobs, 16):
            oc = c[None, :] - centres[lo:lo + 16]                                       # [b,3]
            b = 2 * torch.einsum("hwk,bk->bhw", dirs, oc)
            disc = b * b - 4 * a[None] * ((oc * oc).sum(-1) - radius ** 2)[:, None, None]
            t = torch.where(disc > 0, (-b - torch.sqrt(disc.clamp(min=0))) / (2 * a[None]), torch.full_like(b, float("inf")))
            t = torch.where(t > 0, t, torch.full_like(t, float("inf"))).amin(0)
            depth[v] = torch.where((t < depth[v]) | ((depth[v] <= 0) & torch.isfinite(t)), t, depth[v])


def cpu_filter(vertices, faces, share):
    """scipy + numpy on the host -> (kept vertex bytes, kept faces, components with a face)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    nv = len(vertices)
    rows, cols = np.concatenate([faces[:, 0], faces[:, 0]]), np.concatenate([faces[:, 1], faces[:, 2]])
    _, comp = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(nv, nv)), directed=False)
    count = np.bincount(comp[faces[:, 0]], minlength=comp.max() + 1)
    keep_v = count[comp] >= fusion.mesh_min_faces(0, share, int(count.max()))
    rank = np.cumsum(keep_v) - keep_v
    return vertices[keep_v], rank[faces[keep_v[faces[:, 0]]]].astype(np.int32), int((count > 0).sum())


def one_config(h, w, res, a, dev):
    views = list(mesh_bench.scan(h, w, dev))
    add_blobs(views[0], h, w, a.blobs, a.blob_radius, dev)
    half = mesh_bench.HALF
    plan = fusion.mesh_plan((-half,) * 3 + (half,) * 3, resolution=res, trunc_voxels=3.0, widen=False)
    state = ops.tsdf_volume(plan["dims"], dev)
    for lo in range(0, mesh_bench.N_IMG, fusion.MESH_INTEGRATE_BATCH):
        ops.tsdf_integrate(state, plan["dims"], plan["origin"], plan["voxel"], plan["trunc"], *(t[lo:lo + fusion.MESH_INTEGRATE_BATCH] for t in views))
    box = {}

    def extract():
        box["mesh"] = fusion.extract_mesh(state, plan, 2)

    out = {"shape": f"{w}x{h}", "volume": res, "blobs": a.blobs, "blob_radius": a.blob_radius, "share": a.share}
    out["extract_ms"], out["extract_ms_rounds"] = mesh_bench.timed(extract, a.rounds)
    vertices, faces = box["mesh"]
    del state
    nv, nf = vertices.numel() // ops.MESH_VERTEX_BYTES, faces.numel() // 3

    def components():
        box["cc"] = ops.mesh_components(faces, nv)

    out["components_ms"], out["components_ms_rounds"] = mesh_bench.timed(components, a.rounds)
    label, count, totals = box["cc"]
    n_comp, largest, valid = totals.tolist()
    min_faces = fusion.mesh_min_faces(0, a.share, largest)
    info = {}

    def whole():
        box["kept"] = fusion.keep_mesh_components(vertices, faces, 0, a.share, info=info)

    out["filter_ms"], out["filter_ms_rounds"] = mesh_bench.timed(whole, a.rounds)
    kept_v, kept_f = box["kept"]
    out_v, out_f = torch.empty_like(kept_v), torch.empty_like(kept_f)
    kept = torch.zeros(2, device=dev, dtype=torch.int64)
    workspace = torch.empty(ops.mesh_keep_workspace_bytes(nv, nf), device=dev, dtype=torch.uint8)
    out["keep_ms"], out["keep_ms_rounds"] = mesh_bench.timed(
        lambda: ops.mesh_keep(vertices, ops.MESH_VERTEX_BYTES, faces, label, count, min_faces, out_v, out_f, kept, workspace), a.rounds)
    assert torch.equal(out_v, kept_v) and torch.equal(out_f, kept_f) and kept.tolist() == [info["vertices"], info["faces"]]
    out.update(vertices=nv, faces=nf, valid_faces=valid, components=n_comp, largest=largest, min_faces=min_faces,
               kept_components=info["kept_components"], kept_vertices=info["vertices"], kept_faces=info["faces"],
               filter_bytes=info["component_bytes"],
               download_bytes=nv * ops.MESH_VERTEX_BYTES + nf * ops.MESH_FACE_BYTES,
               download_bytes_saved=(nv - info["vertices"]) * ops.MESH_VERTEX_BYTES + (nf - info["faces"]) * ops.MESH_FACE_BYTES)
    host_v, host_f = vertices.cpu().numpy().reshape(-1, ops.MESH_VERTEX_BYTES), faces.cpu().numpy().reshape(-1, 3)
    seconds = []
    for _ in range(a.cpu_rounds):
        t0 = time.perf_counter()
        cpu = cpu_filter(host_v, host_f, a.share)
        seconds.append(time.perf_counter() - t0)
    assert np.array_equal(cpu[0].reshape(-1), kept_v.cpu().numpy()) and np.array_equal(cpu[1].reshape(-1), kept_f.cpu().numpy())
    assert cpu[2] == n_comp
    out.update(cpu_scipy_numpy_ms=1e3 * statistics.median(seconds), cpu_scipy_numpy_ms_rounds=[1e3 * s for s in seconds],
               cpu_equals_gpu=True)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="profiles/mesh_components")
    p.add_argument("--shape", default="640x512")
    p.add_argument("--volumes", nargs="+", type=int, default=[256, 512])
    p.add_argument("--blobs", type=int, default=200)
    p.add_argument("--blob_radius", type=float, default=4.0)
    p.add_argument("--share", type=float, default=0.05)
    p.add_argument("--rounds", type=int, default=20)
    p.add_argument("--cpu_rounds", type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_components_bench.py measures on the GPU: none found")
    dev = torch.device("cuda")
    os.makedirs(a.out, exist_ok=True)
    w, h = (int(s) for s in a.shape.split("x"))
    results = [one_config(h, w, res, a, dev) for res in a.volumes]
    with open(os.path.join(a.out, f"mesh_components_bench_{a.shape}.json"), "w") as f:
        json.dump(results, f, indent=1)
    for r in results:
        print(json.dumps({k: v for k, v in r.items() if not k.endswith("_rounds")}))


if __name__ == "__main__":
    main()
