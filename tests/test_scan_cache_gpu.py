"""Scan mode on the MI355X: slot kernels, FeatureNet into slots, cached matching (eager and captured), the eval.py driver."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


# -- 1. slot kernels against the direct kernels -----------------------------------------------------------------------
def _proj(b, s, gen):
    """[3,B,S,12] rows [R | t] near the identity: taps stay inside the maps (a fraction falls off the borders)"""
    r = torch.eye(3).expand(3, b, s, 3, 3) + 0.02 * torch.randn(3, b, s, 3, 3, generator=gen)
    t = 0.05 * torch.randn(3, b, s, 3, 1, generator=gen)
    return torch.cat([r, t], -1).reshape(3, b, s, 12).contiguous().to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("s,b", [(1, 1), (4, 2), (10, 1), (16, 2)])
def test_slot_kernels_equal_direct_kernels(dtype, s, b):
    from itermvs_amd import ops
    from itermvs_amd.engine import sample_offsets
    gen = torch.Generator().manual_seed(17 * s + b)
    h, w = 20, 28                               # level-2 grid: neither dimension a multiple of the 16 x 2 tile
    dims = {1: (16, 2 * h, 2 * w), 2: (32, h, w), 3: (48, h // 2, w // 2)}
    n_slots = s + 4
    slab, maps = {}, {}
    for l, (c, hh, ww) in dims.items():
        slab[l] = torch.full((n_slots, c, hh, ww), float("nan"), device=DEV, dtype=dtype).contiguous(memory_format=torch.channels_last)
        maps[l] = torch.randn(s + 1, c, hh, ww, generator=gen).to(DEV, dtype)
    # item b reads image i at slot perm[b][i]; two views of item 0 share one slot (the same image twice); unused slots hold NaN
    slots = []
    for bi in range(b):
        p = torch.randperm(n_slots, generator=gen)[:s].tolist()
        if s > 1 and bi == 0:
            p[1] = p[0]
        slots.append(p)
    dense = {l: [] for l in dims}
    for bi in range(b):
        for si in range(s):
            img = (si + bi) % (s + 1) if not (s > 1 and bi == 0 and si == 1) else (0 + bi) % (s + 1)
            for l in dims:
                slab[l][slots[bi][si]] = maps[l][img]
    for l in dims:
        dense[l] = [torch.stack([slab[l][slots[bi][si]] for bi in range(b)]).contiguous(memory_format=torch.channels_last)
                    for si in range(s)]
    table = torch.tensor(slots, dtype=torch.int32, device=DEV)
    src_slots = {l: ops.SlotSource(slab[l], table) for l in dims}
    proj = _proj(b, s, gen)
    inv_min = torch.tensor([1 / 400.0, 1 / 500.0][:b], device=DEV)
    inv_max = torch.tensor([1 / 900.0, 1 / 1100.0][:b], device=DEV)
    ref_q = torch.randn(b, h, w, 96, generator=gen).to(DEV)
    nd = torch.rand(b, 1, h, w, generator=gen).to(DEV)
    view_w = torch.rand(b, s, h, w, generator=gen).to(DEV)
    offs = sample_offsets()
    want = ops.corr_iter(dense, ref_q, proj, view_w, inv_min, inv_max, norm_depth=nd, offsets=offs)
    got = ops.corr_iter(src_slots, ref_q, proj, view_w, inv_min, inv_max, norm_depth=nd, offsets=offs)
    for g, x in zip(got, want):
        assert torch.isfinite(x).all()
        assert torch.equal(g, x)
    ref3 = torch.randn(b, 48, h // 2, w // 2, generator=gen).to(DEV, dtype).contiguous(memory_format=torch.channels_last)
    for gl in (False, True):
        want = ops.corr_init(dense[3], ref3, proj[2], inv_min, inv_max, 32, groups_last=gl)
        got = ops.corr_init(src_slots[3], ref3, proj[2], inv_min, inv_max, 32, groups_last=gl)
        assert torch.isfinite(want).all() and torch.equal(got, want)


# -- 2. FeatureNet into slots --------------------------------------------------------------------------------------------
def _model(feature_dtype="fp32", arith="bf16x3", projection="device_fp64", seed=0, graphs=False):
    from itermvs_amd import synthetic
    from itermvs_amd.net import Pipeline
    m = Pipeline(iteration=2, test=True)
    m.load_state_dict(synthetic.random_state_dict(seed))
    m.feature_dtype, m.conv_arithmetic, m.projection, m.use_graphs = feature_dtype, arith, projection, graphs
    return m.to(DEV).eval()


@pytest.mark.parametrize("feature_dtype,arith", [("fp32", "bf16x3"), ("fp16", "bf16x3"), ("bf16", "fp32")])
def test_feature_net_into_slots(feature_dtype, arith):
    from itermvs_amd import synthetic
    eng = _model(feature_dtype, arith).inference_engine()
    s = synthetic.make_scene_sample(num_views=3, height=64, width=96, seed=3)
    x = s["imgs"]["level_0"][0].to(DEV).contiguous()
    with torch.no_grad():
        f = eng.feature_net(x)
        want = [f[1].clone(), f[2].clone(), f[3].clone(), eng.o2_planar.clone()]
        slab = eng.new_slab(8, 64, 96)
        for t in (*slab.levels.values(), slab.planar):
            t.fill_(float("nan"))
        eng.features_into(slab, x, [5, 1, 3])
    torch.cuda.synchronize()
    got = [slab.levels[1], slab.levels[2], slab.levels[3], slab.planar]
    for i, slot in enumerate([5, 1, 3]):
        for g, w_ in zip(got, want):
            assert torch.equal(g[slot], w_[i])
    assert torch.isnan(slab.planar[0]).all()                         # untouched slots stay as they were


# -- 3. cached matching against run / Pipeline.forward -------------------------------------------------------------------
def _scene(b, v=4, h=64, w=96):
    from itermvs_amd import synthetic
    if b == 1:
        return synthetic.make_scene_sample(num_views=v, height=h, width=w, seed=5)
    return synthetic.make_scene_batch(num_views=v, height=h, width=w, seeds=(5, 6), depth_ranges=((420.0, 930.0), (440.0, 900.0)))


@pytest.mark.parametrize("arith", ["bf16x3", "fp32"])
@pytest.mark.parametrize("feature_dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("projection", ["device_fp64", "host_fp32"])
@pytest.mark.parametrize("b", [1, 2])
def test_run_cached_equals_run(arith, feature_dtype, projection, b):
    from itermvs_amd.engine import CachedRunner
    model = _model(feature_dtype, arith, projection)
    eng = model.inference_engine()
    smp = _scene(b)
    imgs = smp["imgs"]["level_0"].to(DEV)
    v = imgs.shape[1]
    projs = {l: smp["proj_matrices"][f"level_{l}"].to(DEV) for l in (1, 2, 3)}
    dmin, dmax = smp["depth_min"].to(DEV), smp["depth_max"].to(DEV)
    with torch.no_grad():
        d0, c0 = (t.clone() for t in eng.run(imgs, projs, dmin, dmax))
        slab = eng.new_slab(3 * v, 64, 96)
        # item bi's views at scattered slots
        slots = [[(7 * (bi * v + i) + 2) % (3 * v) for i in range(v)] for bi in range(b)]
        for bi in range(b):
            eng.features_into(slab, imgs[bi], slots[bi])
        d1, c1 = eng.run_cached(slab, [sl[0] for sl in slots], [sl[1:] for sl in slots], projs, dmin, dmax)
        torch.cuda.synchronize()
        assert torch.equal(d1, d0) and torch.equal(c1, c0)
        if projection == "device_fp64":
            runner = CachedRunner(eng, slab, b, v - 1)
            d2, c2 = runner([sl[0] for sl in slots], [sl[1:] for sl in slots], projs, dmin, dmax)
        else:
            comp = eng.compose_host(torch.stack([projs[1], projs[2], projs[3]]).cpu())
            runner = CachedRunner(eng, slab, b, v - 1, host_composed=True)
            d2, c2 = runner([sl[0] for sl in slots], [sl[1:] for sl in slots], comp, dmin, dmax)
        torch.cuda.synchronize()
        assert torch.equal(d2, d0) and torch.equal(c2, c0)
    eng.check_projection_finite()
    if b == 1 and projection == "device_fp64":                     # and Pipeline.forward (the product's eager path)
        with torch.no_grad():
            out = model({"level_0": imgs}, {f"level_{l}": projs[l] for l in (1, 2, 3)}, dmin, dmax)
        assert torch.equal(out["depths_upsampled"], d0)


def test_one_captured_graph_serves_many_reference_views():
    """one CachedRunner replayed for four reference views of a five-image scene, each with its own cameras and depth range,
    equals each view's eager run"""
    from itermvs_amd import synthetic
    from itermvs_amd.engine import CachedRunner
    eng = _model().inference_engine()
    smp = synthetic.make_scene_sample(num_views=5, height=64, width=96, seed=8)
    imgs = smp["imgs"]["level_0"][0].to(DEV)
    pm = {l: smp["proj_matrices"][f"level_{l}"][0].to(DEV) for l in (1, 2, 3)}
    with torch.no_grad():
        slab = eng.new_slab(6, 64, 96)
        eng.features_into(slab, imgs, [4, 0, 2, 5, 1])
        slot_of = [4, 0, 2, 5, 1]
        runner = CachedRunner(eng, slab, 1, 3)
        for r, srcs in [(0, [1, 2, 3]), (2, [4, 1, 0]), (4, [3, 2, 1]), (1, [0, 4, 3])]:
            order = [r] + srcs
            projs = {l: pm[l][order].unsqueeze(0).contiguous() for l in (1, 2, 3)}
            dmin = torch.tensor([400.0 + 10 * r], device=DEV)
            dmax = torch.tensor([950.0 - 5 * r], device=DEV)
            want = [t.clone() for t in eng.run(imgs[order].unsqueeze(0), projs, dmin, dmax)]
            got = runner([slot_of[r]], [[slot_of[i] for i in srcs]], projs, dmin, dmax)
            torch.cuda.synchronize()
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), r
    eng.check_projection_finite()


def test_run_cached_refuses_the_side_branch():
    from itermvs_amd.engine import InferenceEngine
    model = _model()
    eng = InferenceEngine(model.weights(), 2, side_branch=True)
    slab = eng.new_slab(4, 64, 96)
    with pytest.raises(RuntimeError, match="side_branch"):
        eng.run_cached(slab, [0], [[1, 2]], torch.eye(4, device=DEV).expand(3, 1, 3, 4, 4), torch.ones(1, device=DEV),
                       torch.ones(1, device=DEV) * 2)


# -- 4. driver ----------------------------------------------------------------------------------------------------------
def write_scans(root, n=10, hw=(64, 96), singular=None):
    """two scans of ``n`` views; overlapping neighbour lists; view n-1 is never a reference; view 3 has two sources only.
    ``singular`` = (scan index, view): that view's camera file holds a zero extrinsic."""
    from PIL import Image
    from itermvs_amd import synthetic
    h, w = hw
    names = []
    for si in range(2):
        s = synthetic.make_scene_sample(num_views=n, height=h, width=w, seed=20 + si)
        k0, exts = synthetic.camera_parameters(n, h, w, ref_shift=si)
        scan = os.path.join(root, f"scan{si + 1}")
        os.makedirs(os.path.join(scan, "cams_1"))
        os.makedirs(os.path.join(scan, "images"))
        for v in range(n):
            img = ((s["imgs"]["level_0"][0, v].permute(1, 2, 0).numpy() + 1) * 127.5).round().clip(0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(scan, "images", "{:0>8}.png".format(v)))
            e = np.array(exts[v], dtype=np.float64)
            if singular == (si, v):
                e[:] = 0.0
            rows = lambda m: "\n".join(" ".join(repr(float(x)) for x in r) for r in m)
            with open(os.path.join(scan, "cams_1", "{:0>8}_cam.txt".format(v)), "w") as f:
                f.write(f"extrinsic\n{rows(e)}\n\nintrinsic\n{rows(np.array(k0, dtype=np.float64))}\n\n425.0 2.5 192 935.0\n")
        lines = [str(n - 1)]
        for v in range(n - 1):
            srcs = [(v + 1) % n, (v + n - 1) % n, (v + 2) % n, (v + 5) % n]
            if v == 3:
                srcs = srcs[:2]
            lines += [str(v), f"{len(srcs)} " + " ".join(f"{u} 1.0" for u in srcs)]
        with open(os.path.join(scan, "pair.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        names.append(f"scan{si + 1}")
    return names


def _eval(data, out, extra):
    import eval as E
    args = E.build_parser().parse_args(["--dataset", "folder", "--testpath", str(data), "--n_views", "4", "--img_wh", "96", "64",
                                        "--iteration", "2", "--outdir", str(out)] + extra)
    return E.save_depth(args)


def _pfms(out):
    got = {}
    for dp, _, files in os.walk(out):
        for f in files:
            with open(os.path.join(dp, f), "rb") as fh:
                got[os.path.relpath(os.path.join(dp, f), out)] = fh.read()
    return got


@pytest.mark.parametrize("extra", [[], ["--projection", "host_fp32", "--feature_dtype", "fp16"], ["--no_graphs"]])
def test_eval_feature_cache_writes_identical_pfms(tmp_path, extra):
    write_scans(tmp_path / "data")
    n0 = _eval(tmp_path / "data", tmp_path / "plain", extra)
    assert n0 == 18
    want = _pfms(tmp_path / "plain")
    assert len(want) == 36
    for n in ("40", "4"):                     # the whole of both scans / n_views (evicts and recomputes)
        assert _eval(tmp_path / "data", tmp_path / f"cache{n}", ["--feature_cache", n] + extra) == 18
        assert _pfms(tmp_path / f"cache{n}") == want, n


def test_feature_cache_computes_each_image_once(tmp_path):
    import eval as E
    from itermvs_amd.scan_cache import ScanFeatureCache, save_depth_cached
    from itermvs_amd.scan_dataset import ScanFolderDataset
    names = write_scans(tmp_path / "data")
    args = E.build_parser().parse_args(["--dataset", "folder", "--testpath", str(tmp_path / "data"), "--n_views", "4",
                                        "--img_wh", "96", "64", "--iteration", "2", "--outdir", str(tmp_path / "o"),
                                        "--feature_cache", "20"])
    model = E.load_model(args, torch.device(DEV))
    ds = ScanFolderDataset(str(tmp_path / "data"), names, 4, (96, 64))
    cache = ScanFeatureCache(model, 20)
    assert save_depth_cached(args, ds, list(range(len(ds))), model, torch.device(DEV), cache=cache) == 18
    assert cache.computed == 20                    # every image of both scans once (view 9 only ever as a source)
    cache4 = ScanFeatureCache(model, 4)
    args.feature_cache = 4
    save_depth_cached(args, ds, list(range(len(ds))), model, torch.device(DEV), cache=cache4)
    assert cache4.computed > 20


def test_feature_cache_raises_where_the_uncached_run_raises(tmp_path):
    write_scans(tmp_path / "data", singular=(0, 5))
    errs = {}
    for name, extra in (("plain", []), ("cache", ["--feature_cache", "6"])):
        with pytest.raises(AssertionError, match="nan in proj") as e:
            _eval(tmp_path / "data", tmp_path / name, extra)
        errs[name] = (str(e.value), _pfms(tmp_path / name))
    assert errs["plain"][0] == errs["cache"][0]
    assert errs["plain"][1] == errs["cache"][1] and len(errs["plain"][1]) > 0      # the same depth maps were written before it


# -- 5. invalidation ----------------------------------------------------------------------------------------------------
def test_new_weights_drop_cached_pyramids(tmp_path):
    import eval as E
    from itermvs_amd import synthetic
    from itermvs_amd.scan_cache import ScanFeatureCache, save_depth_cached
    from itermvs_amd.scan_dataset import ScanFolderDataset
    names = write_scans(tmp_path / "data")
    base = ["--dataset", "folder", "--testpath", str(tmp_path / "data"), "--n_views", "4", "--img_wh", "96", "64",
            "--iteration", "2"]
    args = E.build_parser().parse_args(base + ["--outdir", str(tmp_path / "a"), "--feature_cache", "20"])
    model = E.load_model(args, torch.device(DEV))
    ds = ScanFolderDataset(str(tmp_path / "data"), names, 4, (96, 64))
    cache = ScanFeatureCache(model, 20)
    idx = list(range(len(ds)))
    save_depth_cached(args, ds, idx, model, torch.device(DEV), cache=cache)
    first = cache.engine
    model.load_state_dict(synthetic.random_state_dict(1))
    args.outdir = str(tmp_path / "b")
    save_depth_cached(args, ds, idx, model, torch.device(DEV), cache=cache)
    assert cache.engine is not first
    # the new weights' results, as the uncached run with them writes them
    ref = E.build_parser().parse_args(base + ["--outdir", str(tmp_path / "c")])
    m2 = E.load_model(ref, torch.device(DEV))
    m2.load_state_dict(synthetic.random_state_dict(1))
    from eval import save_depth_folder
    save_depth_folder(ref, ds, idx, m2, torch.device(DEV))
    assert _pfms(tmp_path / "b") == _pfms(tmp_path / "c")
    assert _pfms(tmp_path / "a") != _pfms(tmp_path / "b")
