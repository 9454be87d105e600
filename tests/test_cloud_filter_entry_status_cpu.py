"""Error statuses of itermvs_cloud_knn_mean and itermvs_cloud_radius_count: every case starts from a valid argument list in HOST
memory and breaks exactly one thing; every expected status is a rejection that precedes any launch, so no GPU is needed and a fully
valid list is never passed."""
import ctypes as C

import pytest

NULL, DIMS = -1, -2
_BUF = (C.c_double * 64)()
A = C.addressof(_BUF)
INF, NAN = float("inf"), float("nan")

VALID = {
    "itermvs_cloud_knn_mean": dict(xyz_sorted=A, keys_sorted=A, perm=A, n=40, index=None, n_index=0, ox=0.0, oy=0.0, oz=0.0, nx=4, ny=4,
                                   nz=4, edge=0.5, k=20, cap=1.0, rings=4, mean=A, flag=A, stream=None),
    "itermvs_cloud_radius_count": dict(xyz_sorted=A, keys_sorted=A, perm=A, n=40, ox=0.0, oy=0.0, oz=0.0, nx=4, ny=4, nz=4, edge=0.5,
                                       r=0.4, limit=3, count=A, stream=None),
}

GRID = [("n 0", dict(n=0), DIMS), ("n above 0x7fffff00", dict(n=0x7fffff01), DIMS), ("edge 0", dict(edge=0.0), DIMS),
        ("edge negative", dict(edge=-1.0), DIMS), ("edge NaN", dict(edge=NAN), DIMS), ("edge Inf", dict(edge=INF), DIMS),
        ("origin NaN", dict(oy=NAN), DIMS), ("origin Inf", dict(oz=INF), DIMS), ("nx 0", dict(nx=0), DIMS), ("ny 0", dict(ny=0), DIMS),
        ("nz 0", dict(nz=0), DIMS), ("nx 2^21 + 1", dict(nx=2 ** 21 + 1), DIMS), ("nz 2^21 + 1", dict(nz=2 ** 21 + 1), DIMS)]

CASES = {
    "itermvs_cloud_knn_mean": [(f"{p} null", {p: None}, NULL) for p in ("xyz_sorted", "keys_sorted", "perm", "mean", "flag")] + GRID + [
        ("k 0", dict(k=0), DIMS), ("k -1", dict(k=-1), DIMS), ("k 33", dict(k=33), DIMS), ("n = k", dict(n=20), DIMS),
        ("n < k", dict(n=7), DIMS), ("n = k at k 32", dict(n=32, k=32), DIMS), ("cap 0", dict(cap=0.0), DIMS),
        ("cap negative", dict(cap=-1.0), DIMS), ("cap NaN", dict(cap=NAN), DIMS), ("cap Inf", dict(cap=INF), DIMS),
        ("rings 0", dict(rings=0), DIMS), ("rings 2^21 + 1", dict(rings=2 ** 21 + 1), DIMS),
        ("index with n_index 0", dict(index=A, n_index=0), DIMS), ("index with n_index n + 1", dict(index=A, n_index=41), DIMS)],
    "itermvs_cloud_radius_count": [(f"{p} null", {p: None}, NULL) for p in ("xyz_sorted", "keys_sorted", "perm", "count")] + GRID + [
        ("r 0", dict(r=0.0), DIMS), ("r negative", dict(r=-0.4), DIMS), ("r NaN", dict(r=NAN), DIMS), ("r Inf", dict(r=INF), DIMS),
        ("limit 0", dict(limit=0), DIMS), ("limit -5", dict(limit=-5), DIMS),
        ("cells far smaller than r: more than 64 rings", dict(edge=0.4 / 64), DIMS)],
}
ALL = [(fn, name, broken, status) for fn, cases in CASES.items() for name, broken, status in cases]


def test_the_tables_cover_every_argument_that_can_be_wrong():
    from itermvs_amd import _lib
    assert set(CASES) == set(VALID)
    for fn, args in VALID.items():
        assert len(_lib.PROTOTYPES[fn][1]) == len(args), fn
        assert all(broken and set(broken) <= set(args) for _, broken, _ in CASES[fn]), fn
    assert _lib.ABI_VERSION == 20                                  # additions: the version stays


@pytest.mark.parametrize("fn,name,broken,status", ALL, ids=[f"{c[0][14:]}: {c[1]}" for c in ALL])
def test_one_broken_argument(fn, name, broken, status):
    from itermvs_amd import _lib
    assert broken, "a fully valid list is never passed"
    assert getattr(_lib.load(), fn)(*dict(VALID[fn], **broken).values()) == status
