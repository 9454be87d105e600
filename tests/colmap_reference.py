"""Plain-numpy restatement of the reference's COLMAP converter arithmetic (colmap_input.py:319-364) for the tests of
itermvs_amd/colmap.py and of the two kernels behind it: vectorised, with sets instead of the reference's list scans, so it runs
at the sizes the GPU tests use.  tests/golden/colmap_cases.npz pins it against the reference's own output.

Inputs are the kernels' inputs: CSR observation lists over dense point indices (``offsets`` int64 [V+1], ``point`` int32, -1 =
no 3-D point), ``xyz`` float64 [P,3], camera centres float64 [V,3], row 2 of the extrinsics float64 [V,4]."""
import numpy as np


def pair_terms(li, lj, xyz, ci, cj, theta0=5.0, sigma1=1.0, sigma2=10.0, dtype=np.float64):
    """the terms of calc_score(i, j) (colmap_input.py:336-352) in list order: one per entry of ``li`` that is not -1 and occurs
    in ``lj``, multiplicity kept.  ``dtype`` = np.longdouble evaluates every operation in extended precision."""
    li = np.asarray(li)
    hit = li[(li >= 0) & np.isin(li, np.asarray(lj))]
    p = xyz[hit].astype(dtype)
    a, b = ci.astype(dtype) - p, cj.astype(dtype) - p
    cos = (a * b).sum(1) / np.sqrt((a * a).sum(1)) / np.sqrt((b * b).sum(1))
    deg = 180 / np.pi if dtype is np.float64 else dtype(180) / np.arccos(dtype(-1))
    theta = deg * np.arccos(np.clip(cos, -1, 1))
    sigma = np.where(theta <= theta0, dtype(sigma1), dtype(sigma2))
    return np.exp(-(theta - dtype(theta0)) * (theta - dtype(theta0)) / (2 * sigma ** 2))


def view_scores(offsets, point, xyz, centre, theta0=5.0, sigma1=1.0, sigma2=10.0, dtype=np.float64):
    """score [V,V]: symmetric, zero diagonal; each pair summed serially in list order like the reference"""
    v = len(offsets) - 1
    lists = [point[offsets[i]:offsets[i + 1]] for i in range(v)]
    score = np.zeros((v, v), dtype)
    for i in range(v):
        for j in range(i + 1, v):
            s = dtype(0)
            for t in pair_terms(lists[i], lists[j], xyz, centre[i], centre[j], theta0, sigma1, sigma2, dtype):
                s = s + t
            score[i, j] = score[j, i] = s
    return score


def observation_depths(offsets, point, xyz, ext_row2, i):
    """z of image i's valid observations, in list order: ((e0 x + e1 y) + e2 z) + e3, each operation rounded once -- the
    kernel's expression; also the products' magnitudes |e0 x| + |e1 y| + |e2 z| + |e3| for the rounding bound"""
    ids = point[offsets[i]:offsets[i + 1]]
    p = xyz[ids[ids >= 0]]
    e = ext_row2[i]
    z = ((e[0] * p[:, 0] + e[1] * p[:, 1]) + e[2] * p[:, 2]) + e[3]
    mag = np.abs(e[0] * p[:, 0]) + np.abs(e[1] * p[:, 1]) + np.abs(e[2] * p[:, 2]) + np.abs(e[3])
    return z, mag


def depth_ranges(offsets, point, xyz, ext_row2):
    """colmap_input.py:319-333 -> (range float64 [V,2], magnitude [V,2] of the selected observations' products)"""
    v = len(offsets) - 1
    out, mags = np.full((v, 2), np.nan), np.full((v, 2), np.nan)
    for i in range(v):
        z, mag = observation_depths(offsets, point, xyz, ext_row2, i)
        if len(z) == 0:
            continue
        order = np.argsort(z, kind="stable")
        for t, q in enumerate((.01, .99)):
            k = order[int(len(z) * q)]
            out[i, t], mags[i, t] = z[k], mag[k]
    return out, mags


def pair_rows(text):
    """pair.txt -> [[(id, "%f" text), ...] per row], checking the row headers"""
    tok = text.split("\n")
    n = int(tok[0])
    rows = []
    for i in range(n):
        assert int(tok[1 + 2 * i]) == i
        el = tok[2 + 2 * i].split()
        assert int(el[0]) == (len(el) - 1) // 2
        rows.append(list(zip([int(x) for x in el[1::2]], el[2::2])))
    return rows


def compare_pair_text(got, want, score, score_floor):
    """the "ties" rule: per row the same count, the same (id, "%f" text) multiset, and identical order for every adjacent pair of
    the reference's entries whose reference scores differ by more than 2 x 32 x score_floor x max(1, score).  Returns the number of
    adjacent pairs whose order was checked."""
    g, w = pair_rows(got), pair_rows(want)
    assert len(g) == len(w)
    checked = 0
    for i, (gr, wr) in enumerate(zip(g, w)):
        assert len(gr) == len(wr), i
        assert sorted(gr) == sorted(wr), i
        pos = {}
        for n, (k, _) in enumerate(gr):
            pos.setdefault(k, n)
        for (ka, _), (kb, _) in zip(wr[:-1], wr[1:]):
            sa, sb = score[i, ka], score[i, kb]
            if abs(sa - sb) > 2 * 32 * score_floor * max(1.0, sa, sb):
                assert pos[ka] < pos[kb], (i, ka, kb)
                checked += 1
    return checked
