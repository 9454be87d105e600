"""Training datasets on the host (itermvs_amd/train_dataset.py): metas and paths of both layouts, projection matrices
against the restated reference (tests/train_input_reference.py), the per-sample draws, sharding, and train.py's flags."""
import os
import random

import numpy as np
import pytest
import torch

import train_input_reference as R


@pytest.fixture(scope="module")
def dtu_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dtu"))
    R.write_dtu_tree(root, scans=("scan1", "scan4"), n_views=5, n_src=4, lights=range(7), depth_hw=(1200, 1600))
    return root


@pytest.fixture(scope="module")
def blended_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("blended"))
    R.write_blended_tree(root, scans=("sceneA", "sceneB"), n_views=6, src_counts=[5, 3, 4, 5, 2, 5])
    return root


def test_dtu_metas_and_paths(dtu_root):
    from itermvs_amd.train_dataset import DTUDataset
    ds = DTUDataset(dtu_root, ["scan1", "scan4"], "train", 5)
    assert len(ds) == 2 * 5 * 7                                          # scans x pair.txt views x 7 lights
    assert ds.metas[0] == ("scan1", 0, 0, [1, 2, 3, 4]) and ds.metas[8] == ("scan1", 1, 1, [2, 3, 4, 0])
    assert ds.metas[35][0] == "scan4"
    p = ds.paths("scan4", 3, 2)
    assert p["image"] == os.path.join(dtu_root, "Rectified/scan4_train/rect_003_3_r5000.png")
    assert p["cam"] == os.path.join(dtu_root, "Cameras_1/scan4_train/00000002_cam.txt")
    assert p["depth"] == os.path.join(dtu_root, "Depths_raw/scan4/depth_map_0002.pfm")
    assert p["mask"] == os.path.join(dtu_root, "Depths_raw/scan4/depth_visual_0002.png")
    assert all(os.path.isfile(f) for f in p.values())
    lst = os.path.join(dtu_root, "list.txt")
    with open(lst, "w") as f:
        f.write("scan1\n")
    assert len(DTUDataset(dtu_root, lst, "val", 5)) == 35


def test_blendedmvs_metas_keep_views_with_enough_sources(blended_root):
    from itermvs_amd.train_dataset import BlendedMVSDataset
    ds = BlendedMVSDataset(blended_root, ["sceneA", "sceneB"], "train", 5)
    # views 1 (3 sources) and 4 (2 sources) have fewer than nviews - 1 = 4
    assert [m[1] for m in ds.metas] == [0, 2, 3, 5] * 2 and ds.metas[1] == ("sceneA", 2, [3, 4, 5, 0])
    assert len(BlendedMVSDataset(blended_root, ["sceneA"], "train", 4)) == 5
    p = ds.paths("sceneB", 3)
    assert p["image"] == os.path.join(blended_root, "sceneB/blended_images/00000003.jpg")
    assert p["depth"] == os.path.join(blended_root, "sceneB/rendered_depth_maps/00000003.pfm")
    assert p["cam"] == os.path.join(blended_root, "sceneB/cams/00000003_cam.txt")
    with pytest.raises(ValueError, match="multiples of 32"):
        BlendedMVSDataset(blended_root, ["sceneA"], "train", 5, img_wh=(760, 576))


def test_blendedmvs_scale_factor_follows_the_fixed_rule(blended_root):
    """100 / depth_min of the scan's first reference view in pair.txt, whatever is read first"""
    from itermvs_amd.train_dataset import BlendedMVSDataset
    ds = BlendedMVSDataset(blended_root, ["sceneB", "sceneA"], "val", 5)
    for scan in ("sceneA", "sceneB"):
        want = 100.0 / R.read_cam(os.path.join(blended_root, scan, "cams", "00000000_cam.txt"))[2]
        assert ds.scale_factors[scan] == want
    ds.item(3, 0)                                                      # reading other views first changes nothing
    assert ds.scale_factors["sceneB"] == 100.0 / R.read_cam(os.path.join(blended_root, "sceneB/cams/00000000_cam.txt"))[2]


@pytest.mark.parametrize("mode", ["val", "train"])
def test_dtu_projection_matrices_equal_the_reference(dtu_root, mode):
    from itermvs_amd.train_dataset import DTUDataset
    ds = DTUDataset(dtu_root, ["scan1", "scan4"], mode, 5)
    for idx in (0, 17, 40):
        views, scale, _ = ds.draws(idx, 3)
        assert (scale == 1) == (mode == "val")
        s = ds.item(idx, 3)
        scan = ds.metas[idx][0]
        for i, v in enumerate(views):
            want = R.dtu_proj(os.path.join(dtu_root, f"Cameras_1/{scan}_train/{v:08d}_cam.txt"), scale)
            for l in range(4):
                got = s["proj_matrices"][f"level_{l}"][i]
                assert got.dtype == np.float32 and np.array_equal(got, want[f"level_{l}"]), (idx, i, l)
        _, _, dmin, dmax = R.read_cam(os.path.join(dtu_root, f"Cameras_1/{scan}_train/{views[0]:08d}_cam.txt"))
        assert (s["depth_min"], s["depth_max"]) == (dmin * scale, dmax * scale)


@pytest.mark.parametrize("mode", ["val", "train"])
def test_blendedmvs_projection_matrices_equal_the_reference(blended_root, mode):
    from itermvs_amd.train_dataset import BlendedMVSDataset
    ds = BlendedMVSDataset(blended_root, ["sceneA", "sceneB"], mode, 5)
    for idx in range(len(ds)):
        views, scale, _ = ds.draws(idx, 1)
        s = ds.item(idx, 1)
        scan = ds.metas[idx][0]
        sf = ds.scale_factors[scan]
        for i, v in enumerate(views):
            want = R.blended_proj(os.path.join(blended_root, scan, "cams", f"{v:08d}_cam.txt"), sf, scale)
            for l in range(4):
                assert np.array_equal(s["proj_matrices"][f"level_{l}"][i], want[f"level_{l}"]), (idx, i, l)
        _, _, dmin, dmax = R.read_cam(os.path.join(blended_root, scan, "cams", f"{views[0]:08d}_cam.txt"))
        assert (s["depth_min"], s["depth_max"]) == (dmin * sf * scale, dmax * sf * scale)
        assert np.array_equal(s["gt_params"], np.array([sf, scale, dmin * sf * scale, dmax * sf * scale], np.float32))


def test_robust_train_and_jitter_draws_are_per_sample_and_follow_torchvision(dtu_root):
    from itermvs_amd.train_dataset import DTUDataset, sample_key
    ds = DTUDataset(dtu_root, ["scan1"], "train", 5, seed=7)
    a, b = ds.draws(4, 2), ds.draws(4, 2)
    assert a == b                                                     # reproducible per (seed, epoch, index)
    assert ds.draws(5, 2) != a and ds.draws(4, 3) != a
    assert DTUDataset(dtu_root, ["scan1"], "train", 5, seed=8).draws(4, 2) != a
    # the sequence: random.sample then random.uniform on one Random; randperm(4) -> brightness -> contrast per view
    key = sample_key(7, 2, 4)
    rnd = random.Random(key)
    srcs = ds.metas[4][3]
    index = rnd.sample(range(len(srcs)), 4)
    assert a[0] == [ds.metas[4][2]] + [srcs[i] for i in index] and a[1] == rnd.uniform(0.8, 1.25)
    gen = torch.Generator().manual_seed(key)
    for draw in a[2]:
        perm = torch.randperm(4, generator=gen).tolist()
        bf = float(torch.empty(1).uniform_(0.5, 1.5, generator=gen))
        cf = float(torch.empty(1).uniform_(0.5, 1.5, generator=gen))
        assert draw == (bf, cf, perm.index(1) < perm.index(0))
        assert 0.5 <= bf <= 1.5 and 0.5 <= cf <= 1.5
    orders = {d[2] for i in range(30) for d in ds.draws(i % len(ds), i)[2]}
    assert orders == {True, False}
    rec = ds.item(4, 2)["jitter"]
    assert [tuple(r) for r in rec.tolist()] == [(np.float32(d[0]), np.float32(d[1]), int(d[2]), 1) for d in a[2]]


def test_val_mode_draws_nothing(dtu_root, blended_root):
    from itermvs_amd.train_dataset import BlendedMVSDataset, DTUDataset
    for ds in (DTUDataset(dtu_root, ["scan1"], "val", 5), BlendedMVSDataset(blended_root, ["sceneA"], "val", 5)):
        state = random.getstate(), torch.get_rng_state()
        for idx in range(len(ds)):
            views, scale, jit = ds.draws(idx, idx)
            ref, srcs = ds.metas[idx][-2:]
            assert views == [ref] + srcs[:4] and scale == 1 and jit == [None] * 5
            assert ds.item(idx, 0)["jitter"]["enabled"].tolist() == [0] * 5
        assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[1])


@pytest.mark.parametrize("world", [1, 2, 8])
def test_shards_cover_the_permutation_with_drop_last(world):
    from itermvs_amd.train_dataset import epoch_batches, epoch_permutation
    n, b = 49 * 7 * 3, 4
    perm = epoch_permutation(n, 1, 5)
    assert sorted(perm) == list(range(n)) and perm == epoch_permutation(n, 1, 5) and perm != epoch_permutation(n, 1, 6)
    shards = [epoch_batches(n, b, world, r, 1, 5) for r in range(world)]
    steps = n // (b * world)
    assert all(len(s) == steps and all(len(x) == b for x in s) for s in shards)
    flat = [i for s in shards for x in s for i in x]
    assert len(flat) == len(set(flat)) == steps * b * world
    assert set(flat) == set(perm[:steps * b * world])
    assert n - len(flat) == n % (b * world)                             # what drop_last leaves out
    val = [epoch_batches(n, b, world, r, 1, 5, train=False) for r in range(world)]
    vflat = sorted(i for s in val for x in s for i in x)
    assert vflat == list(range(n))                                      # no shuffle, nothing dropped
    assert epoch_batches(n, b, world, 0, 1, 5, max_steps=3) == shards[0][:3]


def test_train_parser_accepts_the_datasets():
    import train as T
    p = T.build_parser()
    for name, wh in (("dtu_yao", [640, 512]), ("blendedmvs", [768, 576])):
        a = T.resolve_args(p, p.parse_args(["--dataset", name, "--trainpath", "/d", "--trainlist", "t.txt", "--vallist", "v.txt",
                                            "--num_workers", "2"]))
        assert a.valpath == "/d" and a.img_wh == wh and a.num_workers == 2 and a.steps_per_epoch is None
    a = T.resolve_args(p, p.parse_args([]))
    assert a.dataset == "synthetic" and a.img_wh == [640, 512] and T.synthetic_steps(a) == 8 and a.num_workers == 4
    assert T.synthetic_steps(p.parse_args(["--steps_per_epoch", "3"])) == 3


def test_train_parser_missing_trainpath_is_a_clear_error(capsys):
    import train as T
    p = T.build_parser()
    with pytest.raises(SystemExit):
        T.resolve_args(p, p.parse_args(["--dataset", "dtu_yao", "--trainlist", "t.txt", "--vallist", "v.txt"]))
    assert "--dataset dtu_yao needs --trainpath" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["--dataset", "tanks"])


def test_parsed_arguments_work_without_resolve_args():
    """library callers that parse without resolve_args still get the synthetic defaults (640 x 512, 8 steps)"""
    import train as T
    a = T.build_parser().parse_args(["--n_views", "3", "--batch_size", "1"])
    assert T.image_size(a) == [640, 512] and T.synthetic_steps(a) == 8
    imgs = T.synthetic_batch(a, 0, 0, torch.device("cpu"))[0]
    assert imgs["level_0"].shape == (1, 3, 3, 512, 640)
    assert T.image_size(T.build_parser().parse_args(["--dataset", "blendedmvs"])) == [768, 576]


def test_real_data_validation_reduces_sums_and_counts(monkeypatch):
    """a rank without validation batches still sends every scalar (zeros) and its count; the mean is over batches"""
    import argparse
    import train as T
    args = argparse.Namespace(regress=True, iteration=2)
    keys = T.val_keys(2)
    monkeypatch.setattr(T, "validation_batches", lambda *a, **k: iter(()))
    empty = T.validate(None, args, 1, 1, torch.device("cpu"), dataset=object())
    assert set(empty) == set(keys) and all(v == 0.0 for v in empty.values())
    monkeypatch.setattr(T, "validation_batches", lambda *a, **k: iter([(0, 2, "b0"), (1, 2, "b1")]))
    monkeypatch.setattr(T, "val_step", lambda model, batch, regress, it: {k: (1.0 if batch == "b0" else 3.0) for k in keys})
    means = T.validate(None, args, 0, 1, torch.device("cpu"), dataset=object())
    assert means == {k: 2.0 for k in keys}
