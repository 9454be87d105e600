"""numpy restatement of itermvs_tsdf_integrate and itermvs_tsdf_mesh (include/itermvs_hip.h), step by step in the precision and order
written there: float64 geometry as separate multiplications and additions (numpy's ufuncs do not fuse), float32 sums, integer colour
sums.  The two marching-tetrahedra tables are derived here from the rule in csrc/tsdf_tets.hpp, not copied from it;
tests/test_tsdf_cpu.py compares them with what the library returns."""
import itertools

import numpy as np

STATE = np.dtype([("sum", "<f4"), ("count", "<u2"), ("r", "<u2"), ("g", "<u2"), ("b", "<u2")])      # 12 bytes
VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])   # 15 bytes
MAX_COUNT = 257
DIR_BITS = (1, 2, 4, 3, 5, 6, 7)                 # direction 0..6 = +x +y +z +xy +xz +yz +xyz as corner bits
DIR_OF_BITS = {b: d for d, b in enumerate(DIR_BITS)}


def _odd(p):
    return sum(1 for i in range(len(p)) for j in range(i + 1, len(p)) if p[i] > p[j]) % 2 == 1


def tet_corners():
    """[6][4] cube corners: the chain 0, a, a|b, 7 per axis order, the middle two exchanged for the odd orders"""
    out = []
    for perm in itertools.permutations(range(3)):
        a, b, _ = perm
        q = [0, 1 << a, (1 << a) | (1 << b), 7]
        if _odd(perm):
            q[1], q[2] = q[2], q[1]
        out.append(q)
    return out


def tet_cases():
    """[16] lists of triangles; a triangle = three edges (lower, upper local corner)"""
    e = lambda p, q: (min(p, q), max(p, q))      # noqa: E731
    out = []
    for m in range(16):
        ins = [i for i in range(4) if m >> i & 1]
        outs = [i for i in range(4) if not m >> i & 1]
        tris = []
        if len(ins) in (1, 3):
            i = ins[0] if len(ins) == 1 else outs[0]
            j, k, l = [x for x in range(4) if x != i]
            if _odd((i, j, k, l)):
                j, k = k, j
            tris = [[e(i, j), e(i, k), e(i, l)]] if len(ins) == 1 else [[e(i, j), e(i, l), e(i, k)]]
        elif len(ins) == 2:
            (i, j), (k, l) = ins, outs
            if _odd((i, j, k, l)):
                k, l = l, k
            tris = [[e(i, k), e(i, l), e(j, l)], [e(i, k), e(j, l), e(j, k)]]
        out.append(tris)
    return out


def empty_state(dims):
    return np.zeros(int(np.prod(dims)), STATE)


def state_words(state):
    """the state as the int32 [n,3] array the device holds"""
    return state.view("<i4").reshape(-1, 3)


def _split(dims):
    nx, ny, nz = dims
    idx = np.arange(nx * ny * nz, dtype=np.int64)
    return idx % nx, (idx // nx) % ny, idx // (nx * ny)


def _centres(dims, origin, voxel, shift=(0, 0, 0)):
    return [np.float64(origin[a]) + ((i + shift[a]).astype(np.float64) + 0.5) * np.float64(voxel) for a, i in enumerate(_split(dims))]


def integrate(state, dims, origin, voxel, trunc, depth, mask, cams, rgb):
    """steps 1-7 for the views in order, IN PLACE on ``state`` (STATE [n]); depth [V,H,W] f64, mask [V,H,W] u8, cams [V,21] f32, rgb
    [V,H,W,3] u8"""
    cx, cy, cz = _centres(dims, origin, voxel)
    v_n, h, w = depth.shape
    trunc = np.float64(trunc)
    with np.errstate(all="ignore"):
        for v in range(v_n):
            k, e = cams[v, :9].astype(np.float64), cams[v, 9:].astype(np.float64)
            ok = state["count"] < MAX_COUNT
            px = ((e[0] * cx + e[1] * cy) + e[2] * cz) + e[3]
            py = ((e[4] * cx + e[5] * cy) + e[6] * cz) + e[7]
            pz = ((e[8] * cx + e[9] * cy) + e[10] * cz) + e[11]
            ok &= np.isfinite(pz) & (pz > 0)
            ux = ((k[0] * px + k[1] * py) + k[2] * pz) / pz
            uy = ((k[3] * px + k[4] * py) + k[5] * pz) / pz
            rx, ry = np.rint(ux), np.rint(uy)
            ok &= (rx >= 0) & (rx <= w - 1) & (ry >= 0) & (ry <= h - 1)
            xi, yi = np.where(ok, rx, 0).astype(np.int64), np.where(ok, ry, 0).astype(np.int64)
            ok &= mask[v][yi, xi] != 0
            d = depth[v][yi, xi]
            ok &= np.isfinite(d) & (d > 0)
            sdf = d - pz
            ok &= ~(sdf < -trunc)
            t = np.minimum(np.float64(1.0), sdf / trunc).astype(np.float32)
            state["sum"][ok] = state["sum"][ok] + t[ok]
            for name, c in (("r", 0), ("g", 1), ("b", 2)):
                state[name][ok] += rgb[v][yi, xi, c][ok].astype(np.uint16)
            state["count"][ok] += 1
    return state


def mesh(state, dims, origin, voxel, min_count):
    """-> (vertices VERTEX [nv], faces int32 [nf,3]) in the order of the header"""
    nx, ny, nz = dims
    n = nx * ny * nz
    ix, iy, iz = _split(dims)
    off = np.array([(c & 1) + ((c >> 1) & 1) * nx + (c >> 2) * nx * ny for c in range(8)], np.int64)
    count = state["count"].astype(np.int64)
    valid = count >= min_count
    with np.errstate(all="ignore"):
        f = state["sum"] / state["count"].astype(np.float32)
    inside = valid & (f < 0)
    cells = np.nonzero((ix < nx - 1) & (iy < ny - 1) & (iz < nz - 1))[0]
    cells = cells[np.all(valid[cells[:, None] + off[None, :]], axis=1)]
    m = np.zeros(len(cells), np.int64)
    for c in range(8):
        m |= inside[cells + off[c]].astype(np.int64) << c
    marks = np.zeros((n, 7), bool)
    for lo in range(7):
        for d in range(1, 8):
            if lo & d == 0:
                cross = ((m >> lo) ^ (m >> (lo | d))) & 1 == 1
                marks[cells[cross] + off[lo], DIR_OF_BITS[d]] = True
    number = (np.cumsum(marks.reshape(-1)) - marks.reshape(-1)).reshape(n, 7)      # exclusive: ascending (voxel, direction)

    a, direction = np.nonzero(marks)
    bits = np.array(DIR_BITS)[direction]
    b = a + off[bits]
    fa, fb = f[a].astype(np.float64), f[b].astype(np.float64)
    s = fa / (fa - fb)
    vertices = np.zeros(len(a), VERTEX)
    for axis, (name, i) in enumerate(zip("xyz", (ix, iy, iz))):
        ca = np.float64(origin[axis]) + (i[a].astype(np.float64) + 0.5) * np.float64(voxel)
        cb = np.float64(origin[axis]) + ((i[a] + ((bits >> axis) & 1)).astype(np.float64) + 0.5) * np.float64(voxel)
        vertices[name] = (ca + s * (cb - ca)).astype(np.float32)
    for name, ch in (("red", "r"), ("green", "g"), ("blue", "b")):
        qa = state[ch][a].astype(np.float64) / count[a].astype(np.float64)
        qb = state[ch][b].astype(np.float64) / count[b].astype(np.float64)
        vertices[name] = np.clip(np.rint(qa + s * (qb - qa)), 0, 255).astype(np.uint8)

    corners, cases = tet_corners(), tet_cases()
    keys, tris = [], []
    for t in range(6):
        lm = np.zeros(len(cells), np.int64)
        for p in range(4):
            lm |= ((m >> corners[t][p]) & 1) << p
        for case in range(1, 15):
            sel = np.nonzero(lm == case)[0]
            if len(sel) == 0:
                continue
            for j, tri in enumerate(cases[case]):
                cols = []
                for p, q in tri:
                    lo, hi = corners[t][p], corners[t][q]
                    cols.append(number[cells[sel] + off[lo & hi], DIR_OF_BITS[lo ^ hi]])
                keys.append(cells[sel] * 12 + t * 2 + j)
                tris.append(np.stack(cols, axis=1))
    if not keys:
        return vertices, np.zeros((0, 3), np.int32)
    keys, tris = np.concatenate(keys), np.concatenate(tris)
    return vertices, tris[np.argsort(keys, kind="stable")].astype(np.int32)


def sdf_state(dims, origin, voxel, fn, colour=(200, 120, 40)):
    """a volume whose every voxel is valid (count 1) and holds float32(fn(x, y, z)) of its centre"""
    state = empty_state(dims)
    x, y, z = _centres(dims, origin, voxel)
    state["sum"] = fn(x, y, z).astype(np.float32)
    state["count"] = 1
    state["r"], state["g"], state["b"] = colour
    return state


def topology(faces):
    """-> (edge use counts as a dict's values array, V - E + F over the referenced vertices)"""
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64), axis=1)
    _, uses = np.unique(e, axis=0, return_counts=True)
    return uses, len(np.unique(faces)) - len(uses) + len(faces)
