"""fusion.fuse_scan on the MI355X over the cross product of its options, which no other test covers together: dedupe x normals x
consistency, each with all reference views in one flush group and with one view per group, the masks always written, the mesh
written for half of the runs.  What must not depend on the grouping, on the mesh or on the normals is compared between the runs;
the bit-for-bit comparisons against the oracle and the restatements are in the tests of each option."""
import itertools
import os
import re

import numpy as np
import pytest

from test_fuse_claim_cpu import _scan
from test_fusion import _scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, VIEWS = 27, 40, 4                                # ragged against the 32 x 8 tile in both directions
THRES = (1.0, 0.01, 0.3, 2)                            # as tests/test_fuse_claim_gpu.py fuses this scene
MESH = dict(bounds=(-150.0, -100.0, 650.0, 150.0, 100.0, 750.0), resolution=24, min_component=1)
COMBOS = list(itertools.product((False, True), repeat=3))                           # (dedupe, normals, dynamic)
GROUPINGS = ("one_group", "one_view_per_group")


def scan_args():
    """the plane scene of tests/test_fuse_claim_gpu.py's ``scan`` fixture, cut to 4 views of 27 x 40.  On the CPU
    (tests/fuse_claim_reference.py, tests/fuse_dynamic_reference.py) it emits 2365 of 4320 pixels with the static rule, 1091 with
    dedupe, 712 with the dynamic rule and 492 with both."""
    return _scan(_scene(H, W, VIEWS, 4, 0.003))


def run(args, folder, dedupe, normals, dynamic, grouping, mesh):
    """one ``fuse_scan`` into ``folder`` (cloud.ply, mask/, mesh.ply with ``mesh``) -> (shares, info)"""
    from itermvs_amd import fusion
    os.makedirs(folder)
    rec = 27 if normals else 15
    info = {}
    stats = fusion.fuse_scan(*args, os.path.join(folder, "cloud.ply"), *THRES[:3], geo_mask_thres=THRES[3], device=DEV,
                             records_budget=H * W * rec if grouping == "one_view_per_group" else 2 << 30,
                             mask_folder=os.path.join(folder, "mask"), info=info, dedupe=dedupe, normals=normals,
                             mesh=dict(MESH, path=os.path.join(folder, "mesh.ply")) if mesh else None,
                             consistency="dynamic" if dynamic else "static")
    return stats, info


def run_all(root):
    """the 16 runs (every combination in both groupings, the mesh on where ``normals`` is: neither changes what the other writes) and,
    for the direct comparison, the 4 mesh runs once more without the mesh -> {(dedupe, normals, dynamic, grouping, mesh): (folder, shares, info)}"""
    args = scan_args()
    out = {}
    keys = [(*combo, grouping, combo[1]) for combo, grouping in itertools.product(COMBOS, GROUPINGS)]
    keys += [(*combo, "one_group", False) for combo in COMBOS if combo[1]]
    for key in keys:
        folder = os.path.join(root, "dedupe{:d}_normals{:d}_dynamic{:d}_{}_mesh{:d}".format(*key))
        out[key] = (folder, *run(args, folder, *key))
    return out


def files_of(folder):
    """{relative name: bytes} of everything a run wrote"""
    found = {}
    for base, _, names in os.walk(folder):
        for name in names:
            with open(os.path.join(base, name), "rb") as f:
                found[os.path.relpath(os.path.join(base, name), folder)] = f.read()
    return found


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    got = run_all(str(tmp_path_factory.mktemp("options")))
    return {key: (files_of(folder), shares, info) for key, (folder, shares, info) in got.items()}


def _body(ply):
    head, body = ply.split(b"end_header\n", 1)
    return int(re.search(rb"element vertex (\d+)", head).group(1)), body


def test_the_scene_exercises_every_option(runs):
    """not vacuous: the static cloud has vertices, dedupe removes some, the dynamic rule accepts some"""
    count = lambda dedupe, dynamic: runs[(dedupe, False, dynamic, "one_group", False)][2]["vertices"]      # noqa: E731
    print("vertices: static", count(False, False), "dedupe", count(True, False), "dynamic", count(False, True), "both", count(True, True))
    assert 0 < count(True, False) < count(False, False) and 0 < count(True, True) < count(False, True)
    assert len(runs) == 20 and sum(1 for key in runs if key[4]) == 8


@pytest.mark.parametrize("dedupe,normals,dynamic", COMBOS)
def test_the_grouping_changes_nothing(runs, dedupe, normals, dynamic):
    (one, shares_one, info_one), (per, shares_per, info_per) = (runs[(dedupe, normals, dynamic, g, normals)] for g in GROUPINGS)
    assert info_one["groups"] == [(0, VIEWS)] and info_per["groups"] == [(i, i + 1) for i in range(VIEWS)]
    for info in (info_one, info_per):
        assert info["synchronisations"] == len(info["groups"]) == info["downloads"]
    masks = sorted(name for name in one if name.startswith("mask"))
    assert len(masks) == 3 * VIEWS and sorted(one) == sorted(per) == sorted(["cloud.ply"] + masks + ["mesh.ply"] * normals)
    for name in one:                                   # the cloud, every mask and, where it is written, the mesh
        assert one[name] == per[name], name
    assert shares_one == shares_per and list(shares_one) == list(range(VIEWS))
    n, body = _body(one["cloud.ply"])
    assert n == info_one["vertices"] == info_per["vertices"] and len(body) == n * (27 if normals else 15)


@pytest.mark.parametrize("dedupe,dynamic", list(itertools.product((False, True), repeat=2)))
def test_the_mesh_and_the_normals_change_nothing_else(runs, dedupe, dynamic):
    with_mesh, shares_mesh, info_mesh = runs[(dedupe, True, dynamic, "one_group", True)]
    without, shares_without, _ = runs[(dedupe, True, dynamic, "one_group", False)]
    plain, shares_plain, _ = runs[(dedupe, False, dynamic, "one_group", False)]
    assert with_mesh["mesh.ply"].startswith(b"ply\n") and info_mesh["mesh"]["faces"] > 0 and "mesh.ply" not in without
    assert {k: v for k, v in with_mesh.items() if k != "mesh.ply"} == without and shares_mesh == shares_without
    n, body = _body(without["cloud.ply"])
    records = np.frombuffer(body, np.uint8).reshape(n, 27)
    assert _body(plain["cloud.ply"]) == (n, np.delete(records, np.s_[12:24], axis=1).tobytes())
    assert (records[:, 12:24] != 0).any() and shares_plain == shares_without
    assert {k: v for k, v in plain.items() if k != "cloud.ply"} == {k: v for k, v in without.items() if k != "cloud.ply"}


@pytest.mark.parametrize("normals,dynamic", list(itertools.product((False, True), repeat=2)))
def test_the_dedupe_vertices_are_a_sub_sequence(runs, normals, dynamic):
    rec = 27 if normals else 15
    rows = lambda dedupe: np.frombuffer(_body(runs[(dedupe, normals, dynamic, "one_group", normals)][0]["cloud.ply"])[1], np.dtype((np.void, rec)))      # noqa: E731
    some, every = [r.tobytes() for r in rows(True)], iter(r.tobytes() for r in rows(False))
    assert all(r in every for r in some)               # ``in`` consumes the iterator: each vertex is found after the previous one
