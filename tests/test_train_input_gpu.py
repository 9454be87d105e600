"""GPU training input side (itermvs_amd/train_dataset.py, csrc/train_input.hip): Pillow's ColorJitter fused into the image
pyramid, the ground-truth pyramids, whole batches against the restated reference sample (tests/train_input_reference.py),
the prefetching loader and train.py on DTU / BlendedMVS trees.  Every comparison is exact (0 differing values)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import train_input_reference as R

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _images(hw, seed):
    rng = np.random.default_rng(seed)
    h, w = hw
    rand = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    const = np.empty((h, w, 3), np.uint8)
    const[:] = rng.integers(0, 256, 3, dtype=np.uint8)
    sat = np.where(rng.random((h, w, 3)) < 0.85, 255, rng.integers(0, 256, (h, w, 3))).astype(np.uint8)
    return [rand, const, sat]


def _draws(seed):
    fixed = [(f, f) for f in (0.5, 1.0, 1.5)] + [(0.5, 1.5), (1.5, 0.5), (1.0, 1.5), (1.5, 1.0)]
    g = torch.Generator().manual_seed(seed)
    drawn = [(float(torch.empty(1).uniform_(0.5, 1.5, generator=g)), float(torch.empty(1).uniform_(0.5, 1.5, generator=g)))
             for _ in range(16)]
    return [(b, c, cf) for b, c in fixed + drawn for cf in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("src_hw,dst_hw", [((512, 640), (512, 640)), ((576, 768), (576, 768)), ((61, 97), (61, 97)),
                                           ((576, 768), (512, 640))])
def test_jitter_pyramid_equals_pillow_then_image_pyramid(src_hw, dst_hw):
    """level 0 (and the lower levels where the size allows them) == ops.image_pyramid of the bytes PIL.ImageEnhance makes
    for the same factors and order: both orders, factors 0.5 / 1.0 / 1.5 and 16 drawn, random / constant / saturated
    images, plus a view without jitter"""
    from itermvs_amd import ops
    from itermvs_amd.train_dataset import jitter_records
    imgs, draws = _images(src_hw, 3), _draws(4)
    raws, jit = [], []
    for img in imgs:
        for d in draws + [None]:
            raws.append(img)
            jit.append(d)
    raw = torch.from_numpy(np.stack(raws)).to(DEV)
    rec = torch.from_numpy(jitter_records(jit).view(np.uint8)).to(DEV)
    all_levels = dst_hw[0] % 8 == 0 and dst_hw[1] % 8 == 0
    got = ops.image_pyramid_jitter(raw, dst_hw[0], dst_hw[1], rec, all_levels=all_levels)
    want_bytes = np.stack([R.pil_jitter(r, d) for r, d in zip(raws, jit)])
    want = ops.image_pyramid(torch.from_numpy(want_bytes).to(DEV), dst_hw[0], dst_hw[1], all_levels=all_levels)
    assert set(got) == set(want)
    for k in want:
        diff = int((got[k] != want[k]).sum())
        print(src_hw, dst_hw, k, "differing values", diff)
        assert torch.equal(got[k], want[k]), (k, diff)
    # a jitter that changes nothing (f = 1) and the disabled record both reproduce the plain pyramid bit for bit
    plain = ops.image_pyramid(raw, dst_hw[0], dst_hw[1], all_levels=all_levels)
    for i, d in enumerate(jit):
        if d is None or d[:2] == (1.0, 1.0):
            assert torch.equal(got["level_0"][i], plain["level_0"][i])


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 1.1372618])
def test_dtu_ground_truth_equals_the_reference(scale):
    """dtu_yao.py:80-119 at the real sizes (1600 x 1200 depth and depth_visual -> 640 x 512 and its levels)"""
    from itermvs_amd import _lib, ops
    rng = np.random.default_rng(5)
    b, h, w = 2, 1200, 1600
    depth = (rng.random((b, h, w)) * 900 + 100).astype(np.float32)
    depth[:, ::7, ::5] = 0
    visual = rng.integers(0, 30, (b, h, w), dtype=np.uint8)
    rows = np.ascontiguousarray(depth[:, ::-1])                       # as a PFM stores them: bottom-up
    params = np.array([[np.float32(scale), 1, 0, 0]] * b, np.float32)
    got_d, got_m = ops.gt_pyramid(torch.from_numpy(rows).to(DEV), torch.from_numpy(visual).to(DEV),
                                  torch.from_numpy(params).to(DEV), 512, 640, _lib.GT_DTU)
    for i in range(b):
        want_d, want_m = R.dtu_depth_mask(depth[i], visual[i], scale)
        for l in range(4):
            k = f"level_{l}"
            assert got_d[k][i, 0].shape == want_d[k].shape == (512 >> l, 640 >> l)
            assert torch.equal(got_d[k][i, 0].cpu(), torch.from_numpy(want_d[k])), (i, k)
            assert torch.equal(got_m[k][i, 0].cpu(), torch.from_numpy(want_m[k])), (i, k)


@pytest.mark.gpu
@pytest.mark.parametrize("file_hw,img_wh,scale", [((576, 768), (768, 576), 1), ((576, 768), (768, 576), 0.8637211),
                                                  ((576, 768), (640, 512), 1.2012345), ((1152, 1536), (768, 576), 1)])
def test_blendedmvs_ground_truth_equals_the_reference(file_hw, img_wh, scale):
    """blendedmvs.py:62-83: depth resized to img_wh and then to the levels, the mask straight from the file size.  With
    img_wh != the file size the mask's direct map and the depth's two-step map differ (the cv2 map is restated, unpinned)"""
    from itermvs_amd import _lib, ops
    rng = np.random.default_rng(6)
    b = 2
    sf = 100.0 / 2.3
    depth = (rng.random((b,) + file_hw) * 7 + 0.5).astype(np.float32)
    dmin, dmax = 2.3 * sf * scale, 6.9 * sf * scale
    rows = np.ascontiguousarray(depth[:, ::-1])
    params = np.array([[sf, scale, dmin, dmax]] * b, np.float32)
    got_d, got_m = ops.gt_pyramid(torch.from_numpy(rows).to(DEV), None, torch.from_numpy(params).to(DEV), img_wh[1], img_wh[0],
                                  _lib.GT_BLENDEDMVS)
    for i in range(b):
        want_d, want_m = R.blended_depth_mask(depth[i], sf, scale, dmin, dmax, img_wh)
        for l in range(4):
            k = f"level_{l}"
            assert torch.equal(got_d[k][i, 0].cpu(), torch.from_numpy(want_d[k])), (i, k)
            assert torch.equal(got_m[k][i, 0].cpu(), torch.from_numpy(want_m[k])), (i, k)
            assert 0 < float(got_m[k].mean()) < 1


def _reference_batch(ds, idxs, epoch, kind):
    """the reference's collated sample for these draws: PIL jitter -> ops.image_pyramid, restated projections and ground
    truth, float32 depth range"""
    from itermvs_amd import ops
    from itermvs_amd.data_io import read_pfm
    imgs, projs, dmins, dmaxs, depth, mask = {f"level_{l}": [] for l in range(4)}, {f"level_{l}": [] for l in range(4)}, [], [], \
        {f"level_{l}": [] for l in range(4)}, {f"level_{l}": [] for l in range(4)}
    w, h = ds.img_wh
    for idx in idxs:
        views, scale, jit = ds.draws(idx, epoch)
        scan = ds.metas[idx][0]
        raws, pms = [], {f"level_{l}": [] for l in range(4)}
        for i, v in enumerate(views):
            if kind == "dtu":
                p = ds.paths(scan, ds.metas[idx][1], v)
                pm = R.dtu_proj(p["cam"], scale)
            else:
                p = ds.paths(scan, v)
                pm = R.blended_proj(p["cam"], ds.scale_factors[scan], scale)
            from PIL import Image
            raws.append(R.pil_jitter(np.asarray(Image.open(p["image"]).convert("RGB")), jit[i]))
            for l in range(4):
                pms[f"level_{l}"].append(pm[f"level_{l}"])
            if i == 0:
                _, _, dmin, dmax = R.read_cam(p["cam"])
                d_file = np.squeeze(read_pfm(p["depth"])[0], 2)
                if kind == "dtu":
                    dmin, dmax = dmin * scale, dmax * scale
                    dd, mm = R.dtu_depth_mask(d_file, np.asarray(Image.open(p["mask"])), scale, ds.img_wh)
                else:
                    sf = ds.scale_factors[scan]
                    dmin, dmax = dmin * sf * scale, dmax * sf * scale
                    dd, mm = R.blended_depth_mask(d_file, sf, scale, dmin, dmax, ds.img_wh)
                dmins.append(dmin)
                dmaxs.append(dmax)
                for l in range(4):
                    depth[f"level_{l}"].append(dd[f"level_{l}"][None])
                    mask[f"level_{l}"].append(mm[f"level_{l}"][None])
        for k in projs:
            projs[k].append(np.stack(pms[k]))
        pyr = ops.image_pyramid(torch.from_numpy(np.stack(raws)).to(DEV), h, w)
        for k in imgs:
            imgs[k].append(pyr[k])
    stack = lambda d: {k: torch.from_numpy(np.stack(v)).to(DEV) for k, v in d.items()}  # noqa: E731
    return ({k: torch.stack(v) for k, v in imgs.items()}, stack(projs), torch.tensor(dmins, dtype=torch.float32, device=DEV),
            torch.tensor(dmaxs, dtype=torch.float32, device=DEV), stack(depth), stack(mask))


def _assert_batches_equal(got, want):
    names = ["imgs", "proj_matrices", "depth_min", "depth_max", "depth", "mask"]
    for name, g, w in zip(names, got, want):
        if isinstance(w, dict):
            assert set(g) == set(w), name
            for k in w:
                assert g[k].shape == w[k].shape and g[k].dtype == w[k].dtype, (name, k, g[k].shape, w[k].shape)
                assert torch.equal(g[k], w[k]), (name, k, int((g[k] != w[k]).sum()))
        else:
            assert g.dtype == w.dtype and torch.equal(g, w), name


@pytest.fixture(scope="module")
def dtu_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dtu"))
    R.write_dtu_tree(root, scans=("scan1",), n_views=5, n_src=4)
    return root


@pytest.fixture(scope="module")
def blended_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("blended"))
    R.write_blended_tree(root, scans=("sceneA",), n_views=6)
    return root


@pytest.mark.gpu
@pytest.mark.parametrize("kind,mode", [("dtu", "train"), ("dtu", "val"), ("blended", "train"), ("blended", "val")])
def test_whole_batch_equals_the_reference_sample(dtu_tree, blended_tree, kind, mode):
    """to_device of a B = 2 batch == the restated reference sample for the same draws, every tensor of the 6-tuple"""
    from itermvs_amd.train_dataset import BlendedMVSDataset, DTUDataset, collate, to_device
    ds = DTUDataset(dtu_tree, ["scan1"], mode, 5) if kind == "dtu" else BlendedMVSDataset(blended_tree, ["sceneA"], mode, 5)
    idxs, epoch = [3, len(ds) - 2], 2
    got = to_device(collate([ds.item(i, epoch) for i in idxs]), torch.device(DEV), ds.img_wh, ds.recipe)
    want = _reference_batch(ds, idxs, epoch, kind)
    _assert_batches_equal(got, want)
    assert got[0]["level_0"].shape == (2, 5, 3, ds.img_wh[1], ds.img_wh[0]) and got[4]["level_2"].shape == (2, 1, ds.img_wh[1] // 4, ds.img_wh[0] // 4)


@pytest.mark.gpu
def test_loader_is_ordered_whatever_the_thread_count_and_stages_ahead(dtu_tree):
    from itermvs_amd.train_dataset import DTUDataset, TrainPrefetcher, epoch_batches
    ds = DTUDataset(dtu_tree, ["scan1"], "train", 5)
    batches = epoch_batches(len(ds), 2, 1, 0, 1, 0, max_steps=5)
    runs = {}
    for nw in (1, 4):
        pf = TrainPrefetcher(ds, batches, torch.device(DEV), num_workers=nw, epoch=0)
        time.sleep(1.0)                                  # decoding is not the bottleneck here
        out = []
        for _, t in pf:
            time.sleep(0.2)
            torch.cuda.current_stream().synchronize()
            out.append(t)
        assert len(out) == 5 and pf.staged_ahead > 0, pf.staged_ahead
        assert not pf.thread.is_alive()
        runs[nw] = out
    for a, b in zip(runs[1], runs[4]):
        _assert_batches_equal(a, b)


def _run(args, timeout=900):
    env = dict(os.environ)
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _check_scalars(out, key):
    line = [l for l in out.splitlines() if l.startswith(key)][-1]
    means = eval(line[len(key):].strip(), {"inf": float("inf"), "nan": float("nan")})       # printed dict of floats
    assert means and all(np.isfinite(v) for v in means.values()), means
    return means


def _load_in_eval(path):
    import eval as E
    eargs = E.build_parser().parse_args(["--n_views", "3", "--img_wh", "96", "64", "--iteration", "2", "--loadckpt", path])
    E.load_model(eargs, torch.device(DEV))


@pytest.mark.gpu
def test_train_driver_on_dtu_graph_then_val(dtu_tree, tmp_path):
    """train.py --dataset dtu_yao --graph --regress --batch_size 2 --epochs 1 on a 1-scan DTU tree (35 samples), then --mode val
    on its checkpoint.  For test time the command adds --iteration 2 and --steps_per_epoch 6: the epoch runs 6 of its 17 steps
    (three eager warm-up steps, the capture, two replays) and validation 6 of its 18 batches (12 of the 35 samples)."""
    lst = tmp_path / "list.txt"
    lst.write_text("scan1\n")
    log = tmp_path / "log"
    base = ["train.py", "--dataset", "dtu_yao", "--trainpath", dtu_tree, "--trainlist", str(lst), "--vallist", str(lst),
            "--regress", "--batch_size", "2", "--iteration", "2", "--steps_per_epoch", "6", "--logdir", str(log)]
    out = _run(base + ["--graph", "--epochs", "1", "--summary_freq", "1"])
    losses = [float(l.split("train loss = ")[1].split(",")[0]) for l in out.splitlines() if "train loss = " in l]
    assert len(losses) == 6 and all(np.isfinite(losses)), losses
    _check_scalars(out, "avg_test_scalars:")
    ckpt = log / "model_000000.ckpt"
    assert ckpt.is_file()
    _load_in_eval(str(ckpt))
    out = _run(base + ["--mode", "val", "--loadckpt", str(ckpt)])
    _check_scalars(out, "final")


@pytest.mark.gpu
def test_train_driver_on_blendedmvs_eager(blended_tree, tmp_path):
    """train.py --dataset blendedmvs without --graph (--iteration 2 for test time): the whole epoch (6 samples, 3 steps) and
    the whole validation, then --mode val on the checkpoint"""
    lst = tmp_path / "list.txt"
    lst.write_text("sceneA\n")
    log = tmp_path / "log"
    out = _run(["train.py", "--dataset", "blendedmvs", "--trainpath", blended_tree, "--trainlist", str(lst), "--vallist", str(lst),
                "--regress", "--batch_size", "2", "--iteration", "2", "--epochs", "1", "--logdir", str(log), "--summary_freq", "1"])
    losses = [float(l.split("train loss = ")[1].split(",")[0]) for l in out.splitlines() if "train loss = " in l]
    assert len(losses) == 3 and all(np.isfinite(losses)), losses            # 6 samples // 2
    _check_scalars(out, "avg_test_scalars:")
    assert (log / "model_000000.ckpt").is_file()
    _load_in_eval(str(log / "model_000000.ckpt"))
    out = _run(["train.py", "--dataset", "blendedmvs", "--mode", "val", "--valpath", blended_tree, "--vallist", str(lst),
                "--regress", "--batch_size", "2", "--iteration", "2", "--loadckpt", str(log / "model_000000.ckpt")])
    _check_scalars(out, "final")
