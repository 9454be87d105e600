"""``cloud_grid.sort_into_cells`` on the MI355X against a numpy restatement of the cell key: fp64 floor((p - origin) / edge) per
axis, key = (cx * ny + cy) * nz + cz, INT64_MAX for a row that is not finite or lies outside the box."""
import numpy as np
import pytest
import torch

from itermvs_amd import cloud_grid as CG

pytestmark = pytest.mark.gpu
DEV = "cuda"
NO_KEY = np.iinfo(np.int64).max


def restated_keys(pts, grid):
    with np.errstate(invalid="ignore"):
        c = np.floor((pts.astype(np.float64) - np.array(grid.origin)) / grid.edge)
        inside = ((c >= 0) & (c < np.array(grid.dims, dtype=np.float64))).all(1)             # NaN, +-Inf: false
    c = np.where(inside[:, None], c, 0.0).astype(np.int64)
    return np.where(inside, (c[:, 0] * grid.dims[1] + c[:, 1]) * grid.dims[2] + c[:, 2], NO_KEY)


def cloud_with_bad_rows():
    pts = np.random.default_rng(11).uniform(-1.0, 2.0, (305, 3)).astype(np.float32)
    bad = np.array([3, 77, 150, 151, 304])
    pts[bad, [0, 1, 2, 0, 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    return pts, bad


def check_sorted(sc, pts, rows):
    """the properties every mode shares: ``rows`` are the rows of ``pts`` that ``perm`` must be a permutation of"""
    keys, perm, xyz = sc.keys.cpu().numpy(), sc.perm.cpu().numpy(), sc.xyz.cpu().numpy()
    assert sc.xyz.dtype == torch.float32 and sc.keys.dtype == torch.int64 and sc.perm.dtype == torch.int64
    assert sc.xyz.is_contiguous() and xyz.shape == (len(rows), 3) and keys.shape == perm.shape == (len(rows),)
    assert (np.diff(keys) >= 0).all()
    assert np.array_equal(keys, restated_keys(pts, sc.grid)[perm])
    assert np.array_equal(xyz.view(np.int32), pts[perm].view(np.int32))
    assert np.array_equal(np.sort(perm), np.sort(rows))
    return keys, perm


@pytest.mark.parametrize("pad", [0.0, 0.065])
def test_finite_rows_are_sorted_and_perm_indexes_the_tensor_passed_in(pad):
    pts, bad = cloud_with_bad_rows()
    good = np.setdiff1d(np.arange(len(pts)), bad)
    sc = CG.sort_into_cells(torch.from_numpy(pts).to(DEV), 0.13, "test", pad=pad)
    keys, _ = check_sorted(sc, pts, good)
    assert (keys != NO_KEY).all()
    assert sc.grid == CG.grid_for(torch.from_numpy(pts[good]), 0.13, "test", pad)
    all_finite = CG.sort_into_cells(torch.from_numpy(pts[good]).to(DEV), 0.13, "test", pad=pad)
    check_sorted(all_finite, pts[good], np.arange(len(good)))
    assert torch.equal(all_finite.keys, sc.keys) and all_finite.grid == sc.grid


def test_with_an_extent_every_row_is_sorted_and_the_keyless_rows_come_last():
    pts, bad = cloud_with_bad_rows()
    good = np.setdiff1d(np.arange(len(pts)), bad)
    x = torch.from_numpy(pts).to(DEV)
    sc = CG.sort_into_cells(x, 0.13, "test", extent=x[torch.from_numpy(good).to(DEV)])
    keys, perm = check_sorted(sc, pts, np.arange(len(pts)))
    assert (keys[:len(good)] != NO_KEY).all() and (keys[len(good):] == NO_KEY).all()
    assert np.array_equal(np.sort(perm[len(good):]), bad)
    # a box smaller than the cloud: the finite rows outside it are keyless too
    inner = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], device=DEV)
    sc = CG.sort_into_cells(x, 0.13, "test", extent=inner)
    keys, _ = check_sorted(sc, pts, np.arange(len(pts)))
    outside = int((keys == NO_KEY).sum())
    assert len(bad) < outside < len(pts) and sc.grid.origin == (0.0, 0.0, 0.0) and sc.grid.dims == (8, 8, 8)


def test_stable_keeps_the_rows_of_one_cell_in_index_order():
    gen = np.random.default_rng(3)
    places = gen.uniform(0.0, 1.0, (7, 3)).astype(np.float32)
    pts = places[gen.integers(0, 7, 200)]
    sc = CG.sort_into_cells(torch.from_numpy(pts).to(DEV), 0.05, "test", stable=True)
    keys, perm = check_sorted(sc, pts, np.arange(200))
    assert len(np.unique(keys)) == 7
    same = np.diff(keys) == 0
    assert same.sum() == 200 - 7 and (np.diff(perm)[same] > 0).all()


@pytest.mark.parametrize("rows", [0, 4])
@pytest.mark.parametrize("with_extent", [False, True])
def test_no_finite_row_gives_an_empty_cloud_on_one_cell(rows, with_extent):
    x = torch.full((rows, 3), float("nan"), device=DEV)
    if rows:
        x[1, 1], x[2, :2] = float("inf"), 0.5                                                # one bad coordinate is enough
    sc = CG.sort_into_cells(x, 0.25, "test", extent=x[:0] if with_extent else None)
    assert sc.grid == CG.CloudGrid((0.0, 0.0, 0.0), (1, 1, 1), 0.25)
    assert sc.xyz.shape == (0, 3) and sc.xyz.dtype == torch.float32 and sc.xyz.device == x.device
    for t in (sc.keys, sc.perm):
        assert t.shape == (0,) and t.dtype == torch.int64 and t.device == x.device


def test_one_point():
    x = torch.tensor([[float("nan"), 0.0, 0.0], [0.5, -1.25, 3.0]], device=DEV)
    sc = CG.sort_into_cells(x, 0.1, "test")
    assert sc.grid == CG.CloudGrid((0.5, -1.25, 3.0), (1, 1, 1), 0.1)
    assert sc.keys.tolist() == [0] and sc.perm.tolist() == [1] and torch.equal(sc.xyz, x[1:])
    sc = CG.sort_into_cells(x, 0.1, "test", extent=x[1:])
    assert sc.keys.tolist() == [0, NO_KEY] and sc.perm.tolist() == [1, 0]


def test_half_an_edge_of_padding_puts_the_minimum_point_in_cell_zero():
    pts = np.random.default_rng(8).uniform(5.0, 6.0, (300, 3)).astype(np.float32)
    pts[17] = pts.min(0)                                                                     # one row that is the minimum on every axis
    edge = 0.07
    sc = CG.sort_into_cells(torch.from_numpy(pts).to(DEV), edge, "test", pad=edge / 2)
    keys, perm = check_sorted(sc, pts, np.arange(300))
    assert sc.grid.origin == tuple(float(v) - edge / 2 for v in pts.min(0).astype(np.float64))
    assert keys[0] == 0 and 17 in perm[keys == 0]                                            # cell (0, 0, 0)
    assert (np.floor((pts[17].astype(np.float64) - np.array(sc.grid.origin)) / edge) == 0).all()
