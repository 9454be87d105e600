"""The hand-written correlation backward kernels (csrc/corr_bwd.hip) element by element against a float64 reference
(tests/corr_grad_reference.py), and by adjoint identities against the library's own forward.

    itermvs_corr_iter_backward   corr_bwd_kernel: the scatter to the source views (fp32 atomics) + the gather to ref_q
    itermvs_corr_init_backward   corr_bwd_kernel (dL/dref, routed (view, plane) pairs) + init_gather_kernel (dL/dsrc)

Covered: fp32 / bf16 / fp16 storage, 1 .. 16 source views (the iteration branch stages views in chunks of 4), B = 2 with
different cameras per item, map sizes that are not multiples of the 16-pixel tile, behind-camera pixels (sampled at the
sample-grid (W, H), an interior pixel of the level-1 map), a camera sweep through the gather / scatter routing margin of
plane_inverse, the cfg-4 / cfg-5 sizes (persistent grid, xcd_tile) and the shared FeatureGradPool.
Gate of the parity tests: max |got - ref| <= 1e-4 * max(1, max |ref|)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import corr_grad_reference as R
from oracle import itermvs_oracle as O

gpu = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
STORAGE = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}
TOL = 1e-4
NHYP = {1: 4, 2: 4, 3: 2}


def ops():
    from itermvs_amd import ops as _ops
    return _ops


def cu(t):
    return t.to(DEV)


def stored_values(t, storage):
    """the values the kernels read: ``t`` rounded to the storage type, held in fp32"""
    return t if STORAGE[storage] is None else t.to(STORAGE[storage]).float()


def rig_p12(b, v, img_h, img_w, seed):
    """[3,B,S,12] reference-faithful fp32 projections of make_sample's rig (a different rig per batch item)"""
    from itermvs_amd import synthetic
    sm = synthetic.make_sample(b, v, img_h, img_w, seed=seed)
    pr = [sm["proj_matrices"][f"level_{l}"].float() for l in (1, 2, 3)]
    return torch.stack([torch.stack([O.compose_projection(pr[i][:, s], pr[i][:, 0])[:, :3, :4].reshape(-1, 12)
                                     for s in range(1, v)], 1) for i in range(3)]).contiguous()


def put_behind(p12, sizes, bsel):
    """source view 0 of the items ``bsel``: the depth row tilted so that Z of module.py:105 changes sign halfway across
    the sample grid (where exactly depends on the hypothesis' depth); those pixels sample the sample-grid (W, H)"""
    p12 = p12.clone()
    for i, l in enumerate((1, 2, 3)):
        w1 = sizes[l][1]
        p12[i][bsel, 0, 8] = p12[i][bsel, 0, 8] - p12[i][bsel, 0, 10] / (0.5 * w1)
    return p12


def report(name, err, scale, bound=TOL):
    print(f"{name}: {err / scale:.2e} of the scale {scale:.3g} (bound {bound:.0e})")
    return err <= bound * scale


# ---------------------------------------------------------------------------------------------------------------------
# itermvs_corr_iter_backward
# ---------------------------------------------------------------------------------------------------------------------
ITER_CASES = [  # storage, S, B, ragged map, behind-camera rig
    ("fp32", 1, 1, False, False),
    ("bf16", 1, 2, True, True),
    ("fp16", 1, 2, False, False),
    ("fp16", 4, 2, True, False),
    ("fp32", 4, 1, False, True),
    ("bf16", 5, 2, False, False),
    ("fp16", 5, 1, True, True),
    ("fp32", 10, 2, True, False),
    ("fp16", 10, 2, False, True),
    ("bf16", 10, 1, False, False),
    ("fp16", 16, 2, True, False),
    ("fp32", 16, 1, False, False),
    ("bf16", 16, 2, True, True),
]


def _iter_inputs(s, b, ragged, behind, seed):
    v = s + 1
    h, w = (23, 37) if ragged else (24, 40)
    sizes = {1: (2 * h, 2 * w), 2: (h, w), 3: ((h + 1) // 2, (w + 1) // 2)}      # 23x37: 46x74, 23x37, 12x19
    p12 = rig_p12(b, v, 96, 160, seed)
    if behind:
        p12 = put_behind(p12, sizes, slice(None))
    gen = torch.Generator().manual_seed(seed)
    feats = {l: torch.randn((b * v, R.CHANS[l]) + sizes[l], generator=gen) for l in (1, 2, 3)}
    ref_q = torch.randn((b, h, w, 96), generator=gen)
    vw = torch.rand((b, s, h, w), generator=gen)
    nd = torch.rand((b, 1, h, w), generator=gen)
    gout = [torch.randn((b, NHYP[l], 8, h, w), generator=gen) for l in (1, 2, 3)]
    inv_min, inv_max = torch.full((b,), 1 / 425.0), torch.full((b,), 1 / 935.0)
    return dict(v=v, h=h, w=w, sizes=sizes, p12=p12, feats=feats, ref_q=ref_q, vw=vw, nd=nd, gout=gout,
                inv_min=inv_min, inv_max=inv_max)


def _iter_gpu(c, storage, b):
    """corr_iter_train forward on the GPU: (outputs, {l: fp32 feature leaves}, ref_q leaf)"""
    from itermvs_amd.engine import sample_offsets
    fg = {l: cu(c["feats"][l]).contiguous(memory_format=CL).requires_grad_(True) for l in (1, 2, 3)}
    st = None if STORAGE[storage] is None else {l: fg[l].detach().to(STORAGE[storage]) for l in (1, 2, 3)}
    rq = cu(c["ref_q"]).requires_grad_(True)
    outs = ops().corr_iter_train(fg, b, c["v"], rq, cu(c["p12"]), cu(c["vw"]), cu(c["inv_min"]), cu(c["inv_max"]), cu(c["nd"]),
                                 sample_offsets(), stored=st)
    return outs, fg, rq


@gpu
@pytest.mark.parametrize("storage,s,b,ragged,behind", ITER_CASES,
                         ids=[f"{st}-S{s}-B{b}" + ("-ragged" if rg else "") + ("-behind" if bh else "") for st, s, b, rg, bh in ITER_CASES])
def test_corr_iter_backward_against_fp64(storage, s, b, ragged, behind):
    c = _iter_inputs(s, b, ragged, behind, seed=20 + s + 3 * b)
    c["feats"] = {l: stored_values(f, storage) for l, f in c["feats"].items()}      # both sides see the stored values
    v, h, w = c["v"], c["h"], c["w"]
    depth = O.iteration_depth_samples(c["nd"], c["inv_min"].view(b, 1, 1, 1), c["inv_max"].view(b, 1, 1, 1))
    want_out = R.iter_outputs(c["feats"], c["ref_q"], c["p12"], c["vw"], depth, b, v)
    gf_want, grq_want = R.corr_iter_grads(c["feats"], c["ref_q"], c["p12"], c["vw"], depth, c["gout"], b, v)
    outs, fg, rq = _iter_gpu(c, storage, b)
    for i, o in enumerate(outs):
        assert report(f"forward level {i + 1}", *R.parity(o, want_out[i]), 5e-5), i
        assert float((want_out[i] != 0).double().mean()) > 0.1        # the case samples inside the maps
    sum((o * cu(g)).sum() for o, g in zip(outs, c["gout"])).backward()
    ok = True
    for l in (1, 2, 3):
        got = fg[l].grad
        assert got.dtype == torch.float32
        ok &= report(f"dL/dsrc level {l}", *R.parity(got, gf_want[l]))
        assert float(got.reshape(b, v, -1)[:, 0].abs().max()) == 0.0          # the reference view: through ref_q only
        assert float(gf_want[l].abs().max()) > 0.0
    ok &= report("dL/dref_q", *R.parity(rq.grad, grq_want))
    if behind:
        # the patched sample (module.py:106-107): every behind-camera pixel of source view 0 puts weight ~1 on the level-1
        # pixel (W, H) -- an interior pixel of the 2W x 2H map, reached by all of them through atomics
        ph = lambda g: g.reshape(b, v, R.CHANS[1], 2 * h, 2 * w)[:, 1, :, h, w].double().cpu()
        want_p = ph(gf_want[1])
        assert float(want_p.abs().max()) > 1.0, "no behind-camera contribution"
        err = float((ph(fg[1].grad) - want_p).abs().max())
        ok &= report("behind-camera pixel (W, H), level 1", err, max(1.0, float(want_p.abs().max())))
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# itermvs_corr_init_backward
# ---------------------------------------------------------------------------------------------------------------------
def degenerate(p12_3, kind, bi, si=0):
    """camera of source view ``si`` of item ``bi`` made degenerate: ``singular`` (three identical rows: every reference pixel
    lands on one source pixel, no inverse homography) or ``vanishing`` (Z changes sign inside the reference grid)"""
    p = p12_3.clone()
    if kind == "singular":
        p[bi, si, 0:4] = p[bi, si, 8:12]
        p[bi, si, 4:8] = p[bi, si, 8:12]
    elif kind == "vanishing":
        p[bi, si, 8] = -0.1
    return p


def _init_reference_and_gpu(f3, p12_3, b, v, storage, seed):
    h3, w3 = f3.shape[2:]
    inv_min, inv_max = torch.full((b,), 1 / 425.0), torch.full((b,), 1 / 935.0)
    gen = torch.Generator().manual_seed(seed)
    gout = torch.randn((b, v - 1, 32, 8, h3, w3), generator=gen)
    depth = O.initial_depth_samples(inv_min.view(b, 1, 1, 1), inv_max.view(b, 1, 1, 1), h3, w3)
    want = R.corr_init_grads(f3, p12_3, depth, gout, b, v)
    fg = cu(f3).contiguous(memory_format=CL).requires_grad_(True)
    st = None if STORAGE[storage] is None else fg.detach().to(STORAGE[storage])
    out = ops().corr_init_train(fg, b, v, cu(p12_3), cu(inv_min), cu(inv_max), 32, stored=st)
    (out * cu(gout)).sum().backward()
    return fg.grad, want, (gout, depth, inv_min, inv_max, st if st is not None else fg.detach())


INIT_CASES = [  # storage, S, ragged level-3 map, camera made degenerate in the second batch item
    ("fp32", 1, False, "singular"),
    ("bf16", 1, True, "vanishing"),
    ("fp16", 4, True, "singular"),
    ("fp32", 4, False, "vanishing"),
    ("bf16", 10, False, "singular"),
    ("fp16", 10, True, "vanishing"),
    ("fp16", 16, False, "singular"),
    ("bf16", 16, True, None),
    ("fp32", 16, True, "singular"),
]


@gpu
@pytest.mark.parametrize("storage,s,ragged,degen", INIT_CASES,
                         ids=[f"{st}-S{s}" + ("-ragged" if rg else "") + f"-{dg or 'regular'}" for st, s, rg, dg in INIT_CASES])
def test_corr_init_backward_against_fp64(storage, s, ragged, degen):
    b, v = 2, s + 1
    h3, w3 = (12, 19) if ragged else (12, 20)
    p12_3 = rig_p12(b, v, 96, 160, seed=40 + s)[2]
    if degen:
        p12_3 = degenerate(p12_3, degen, bi=1)
    f3 = stored_values(torch.randn((b * v, 48, h3, w3), generator=torch.Generator().manual_seed(s)), storage)
    got, want, _ = _init_reference_and_gpu(f3, p12_3, b, v, storage, seed=s + 1)
    assert float(want.view(b, v, -1)[:, 1:].abs().max()) > 0.0
    assert report(f"init dL/dfeatures {storage} S={s}", *R.parity(got, want))
    # and per part: reference view (gather of corr_bwd_kernel), source views (init_gather_kernel + routed scatter)
    gp, wp = got.reshape(b, v, -1), want.reshape(b, v, -1)
    for part, sl in (("reference view", slice(0, 1)), ("source views", slice(1, v))):
        assert report(f"  {part}", *R.parity(gp[:, sl], wp[:, sl]))


# the camera sweep: a source camera yawed so that the common vanishing line of the 32 fronto-parallel planes (the image of
# the reference's horizontal direction, a vertical line u = cx + f cot(yaw) of the level-3 source map) walks from far
# outside the source image, through the routing margin of plane_inverse (the source image grown by 1.02 px: u = -1.02 and
# u = W1 - 1 + 1.02), into the image.  The camera centre is put on the line through the scene point (0, 0, 600) along its
# optical axis, so part of every plane sweep is imaged.
SWEEP_U = [-2000.0, -60.0, -8.0, -1.5, -1.05, -1.025, -1.0205, -1.0195, -1.015, -1.0, -0.5, 3.0, 9.5,
           18.9, 19.5, 20.0, 20.015, 20.0195, 20.0205, 20.025, 20.05, 21.0, 30.0, 2000.0]
SWEEP_HW = (12, 20)


def sweep_camera(u_h, b=1):
    """[B,1,12] level-3 projection (reference camera = identity extrinsic) of a source camera whose plane vanishing line is
    the source column u_h"""
    from itermvs_amd import synthetic
    h3, w3 = SWEEP_HW
    k0, _ = synthetic.camera_parameters(2, 8 * h3, 8 * w3, 680.0, 0)
    k = k0.copy()
    k[:2] /= 8
    f, cx = k[0, 0], k[0, 2]
    th = math.atan2(f, u_h - cx)                            # cot(th) = (u_h - cx) / f, th in (0, pi)
    rot = np.array([[math.cos(th), 0, -math.sin(th)], [0, 1, 0], [math.sin(th), 0, math.cos(th)]])
    axis = rot[2]                                           # the camera's optical axis in the reference frame
    centre = np.array([0.0, 0.0, 600.0]) - 400.0 * axis
    m = np.concatenate([k @ rot @ np.linalg.inv(k), (k @ (-rot @ centre))[:, None]], 1)   # [K R K^-1 | K t]
    return torch.from_numpy(m.reshape(12)).float().view(1, 1, 12).repeat(b, 1, 1), float(cx + f * math.cos(th) / math.sin(th))


def plane_routed(p12, inv_min, inv_max, w1, h1, n_planes=32):
    """host restatement of plane_inverse (csrc/corr_bwd.hip) for W1 = W: per plane, True when the pair goes to the scatter"""
    m = p12.double().numpy().reshape(12)
    out = []
    for n in range(n_planes):
        d = float(np.float32(1.0) / (np.float32(inv_max) + np.float32(n / (n_planes - 1)) * np.float32(inv_min - inv_max)))
        g = np.array([[d * m[4 * r], d * m[4 * r + 1], d * m[4 * r + 2] + m[4 * r + 3]] for r in range(3)])
        det = np.linalg.det(g)
        nrm = float((g * g).sum())
        if not abs(det) > 1e-13 * nrm * math.sqrt(nrm):
            out.append(True)
            continue
        inv = np.linalg.inv(g).astype(np.float32)
        ws = []
        for cx, cy in ((-1.02, -1.02), (w1 - 1 + 1.02, -1.02), (-1.02, h1 - 1 + 1.02), (w1 - 1 + 1.02, h1 - 1 + 1.02)):
            ws.append(inv.astype(np.float64) @ np.array([cx, cy, 1.0]))
        whole = all(wv[2] * ws[0][2] > 0 and abs(wv[2]) > 1e-5 * np.abs(wv).sum() for wv in ws)
        out.append(not whole)
    return out


def test_sweep_cameras_cross_the_routing_margin():
    """the sweep really passes from pairs the gather serves to pairs routed to the scatter on both sides of the image"""
    served, routed = [], []
    for u in SWEEP_U:
        p, u_got = sweep_camera(u)
        assert abs(u_got - u) <= 1e-6 * max(1.0, abs(u))
        r = plane_routed(p[0, 0], 1 / 425.0, 1 / 935.0, SWEEP_HW[1], SWEEP_HW[0])
        (routed if all(r) else served if not any(r) else routed).append(u)
    print(f"served by the gather: {served}\nrouted to the scatter: {routed}")
    assert -1.05 in served and 20.05 in served and -1.0 in routed and 20.0 in routed and -2000.0 in served


def _init_raw_backward(st3, p12_3, inv_min, inv_max, gout, b, v, depth=None):
    """itermvs_corr_init_backward through the C ABI; ``depth`` [B,32,H,W] explicit planes force the all-atomic scatter"""
    from itermvs_amd import _lib
    o = ops()
    ref3, src3 = o._views(st3, b, v)
    proj, imin, imax = cu(p12_3).contiguous(), cu(inv_min), cu(inv_max)
    p = o._corr_init_params(src3, ref3, proj, imin, imax, 32, None)
    dd = None
    if depth is not None:
        dd = cu(depth).contiguous()
        p.depth = dd.data_ptr()
    gf = torch.zeros_like(st3, dtype=torch.float32)
    gref, gsrc = o._views(gf, b, v)
    ptrs = (C.c_void_p * (v - 1))(*[t.data_ptr() for t in gsrc])
    go = cu(gout).contiguous()
    o.check(_lib.load().itermvs_corr_init_backward(C.byref(p), go.data_ptr(), ptrs, gref.data_ptr(), o._stream()),
            "itermvs_corr_init_backward")
    torch.cuda.synchronize()
    return gf.cpu()


@gpu
@pytest.mark.parametrize("storage", ["fp32", "bf16", "fp16"])
def test_corr_init_backward_camera_sweep(storage):
    """per sweep camera: the generated-plane backward (gather + routed scatter) against the fp64 reference, and against
    the all-atomic scatter of the SAME planes given as explicit depth -- to atomic-order noise, which isolates a missed or
    doubled gather candidate from any oracle / kernel difference"""
    b, v = 2, 3
    h3, w3 = SWEEP_HW
    worst_ref, worst_gs, nonzero = 0.0, 0.0, 0
    base = rig_p12(b, v, 8 * h3, 8 * w3, seed=4)[2]
    for k, u in enumerate(SWEEP_U):
        p12_3 = base.clone()
        p12_3[:, 0] = sweep_camera(u, b)[0][:, 0]                   # source view 0: the sweep camera; view 1: a regular one
        f3 = stored_values(torch.randn((b * v, 48, h3, w3), generator=torch.Generator().manual_seed(100 + k)), storage)
        got, want, (gout, depth, inv_min, inv_max, st3) = _init_reference_and_gpu(f3, p12_3, b, v, storage, seed=200 + k)
        err, scale = R.parity(got, want)
        worst_ref = max(worst_ref, err / scale)
        assert err <= TOL * scale, (u, err / scale)
        gen_ = _init_raw_backward(st3, p12_3, inv_min, inv_max, gout, b, v)
        scat = _init_raw_backward(st3, p12_3, inv_min, inv_max, gout, b, v, depth=depth)
        assert torch.equal(gen_, got.cpu()) or float((gen_ - got.cpu()).abs().max()) <= 1e-5 * scale
        sv = lambda g: g.reshape(b, v, -1)[:, 1].double()             # the sweep view's source gradient
        e_gs = float((sv(gen_) - sv(scat)).abs().max()) / max(1.0, float(sv(scat).abs().max()))
        worst_gs = max(worst_gs, e_gs)
        assert e_gs <= 1e-5, (u, e_gs)
        e_all = float((gen_ - scat).abs().max()) / max(1.0, float(scat.abs().max()))
        assert e_all <= 1e-5, (u, e_all)
        nonzero += int(float(sv(want).abs().max()) > 0.0)
    print(f"camera sweep {storage}: worst vs fp64 {worst_ref:.2e}, worst gather vs scatter {worst_gs:.2e}, "
          f"{nonzero} of {len(SWEEP_U)} cameras with a source gradient")
    assert nonzero >= len(SWEEP_U) - 4


# ---------------------------------------------------------------------------------------------------------------------
# adjoint identities against the library's own forward: sum gout * fwd(delta) == sum grad * delta
# ---------------------------------------------------------------------------------------------------------------------
def _cams(b, v, img_h, img_w):
    from itermvs_amd import synthetic
    lv = {l: [] for l in (1, 2, 3)}
    for bi in range(b):
        cams = synthetic.make_cameras(v, img_h, img_w, ref_shift=7 * bi + 1)
        for l in (1, 2, 3):
            lv[l].append(torch.from_numpy(cams[f"level_{l}"]).float())
    pr = [torch.stack(lv[l]) for l in (1, 2, 3)]
    return torch.stack([torch.stack([O.compose_projection(pr[i][:, s], pr[i][:, 0])[:, :3, :4].reshape(-1, 12)
                                     for s in range(1, v)], 1) for i in range(3)]).contiguous()


def _probes(shape_bv, b, v):
    """localized probes on a [B*V,C,H,W] level (source views 1..V-1 only): name -> mask [B,V,C,H,W] (bool, on the GPU)"""
    _, c, hh, ww = shape_bv
    z = lambda: torch.zeros((b, v, c, hh, ww), dtype=torch.bool, device=DEV)
    out = {}
    m = z()
    m[:, 1:, :, 0, :] = True
    m[:, 1:, :, -1, :] = True
    m[:, 1:, :, :, 0] = True
    m[:, 1:, :, :, -1] = True
    out["border"] = m
    for s in sorted({1, v - 1}):
        m = z()
        m[:, s] = True
        out[f"view{s}"] = m
    m = z()
    m[b - 1, 1:] = True
    out[f"item{b - 1}"] = m
    m = z()
    m[:, 1:, c - 16:] = True
    out["block_last16"] = m
    m = z()
    m[:, 1:] = True
    out["full"] = m
    return out


def _identity(lhs_terms, rhs):
    lhs = float(lhs_terms.sum())
    scale = float(lhs_terms.abs().sum())
    return abs(lhs - rhs), scale


ADJ_SIZES = {"cfg4": (2, 5, 512, 640), "cfg5": (1, 11, 1280, 1920)}


@gpu
@pytest.mark.parametrize("storage", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("size", ["cfg4", "cfg5"])
def test_corr_iter_backward_adjoint_identity(size, storage):
    from itermvs_amd.engine import sample_offsets
    b, v, ih, iw = ADJ_SIZES[size]
    h, w = ih // 4, iw // 4
    sizes = {1: (ih // 2, iw // 2), 2: (h, w), 3: (ih // 8, iw // 8)}
    p12 = put_behind(_cams(b, v, ih, iw), sizes, slice(0, 1))       # item 0, view 0: part of the image behind the camera
    torch.manual_seed(3)
    dt = STORAGE[storage]
    rnd = lambda *shape: torch.randn(shape, device=DEV)
    fg = {l: rnd(b * v, R.CHANS[l], *sizes[l]).contiguous(memory_format=CL).requires_grad_(True) for l in (1, 2, 3)}
    st = None if dt is None else {l: fg[l].detach().to(dt) for l in (1, 2, 3)}
    rq = rnd(b, h, w, 96).requires_grad_(True)
    vw, nd = torch.rand((b, v - 1, h, w), device=DEV), torch.rand((b, 1, h, w), device=DEV)
    inv_min, inv_max = torch.full((b,), 1 / 425.0, device=DEV), torch.full((b,), 1 / 935.0, device=DEV)
    args = (cu(p12), vw, inv_min, inv_max, nd, sample_offsets())
    gout = [rnd(b, NHYP[l], 8, h, w) for l in (1, 2, 3)]
    outs = ops().corr_iter_train(fg, b, v, rq, *args, stored=st)
    sum((o * g).sum() for o, g in zip(outs, gout)).backward()

    def fwd(feats, ref_q):
        with torch.no_grad():
            f32 = {l: (t.float() if dt is not None else t).contiguous(memory_format=CL) for l, t in feats.items()}
            s16 = None if dt is None else {l: t.contiguous(memory_format=CL) for l, t in feats.items()}
            o = ops().corr_iter_train(f32, b, v, ref_q, *args, stored=s16)
        return torch.cat([(oo.double() * g.double()).reshape(-1) for oo, g in zip(o, gout)])

    fails, worst = [], 0.0
    probes = {l: _probes(fg[l].shape, b, v) for l in (1, 2, 3)}
    w1, h1 = w, h                                                     # the behind-camera pixel of level 1: (W, H)
    pix = torch.zeros((b, v, R.CHANS[1]) + sizes[1], dtype=torch.bool, device=DEV)
    pix[0, 1, :, h1, w1] = True
    for name in list(probes[1]) + ["behind_pixel_l1"]:
        delta, rhs = {}, 0.0
        for l in (1, 2, 3):
            if name == "behind_pixel_l1":
                mask = pix if l == 1 else torch.zeros((b, v) + tuple(fg[l].shape[1:]), dtype=torch.bool, device=DEV)
            else:
                mask = probes[l][name]
            d = torch.randn((b, v) + tuple(fg[l].shape[1:]), device=DEV) * mask
            if dt is not None:
                d = d.to(dt)
            delta[l] = d.reshape(fg[l].shape)
            rhs += float((fg[l].grad.double() * delta[l].double()).sum())
        err, scale = _identity(fwd(delta, rq.detach()), rhs)
        worst = max(worst, err / max(scale, 1e-300))
        if not (scale > 0 and err <= 1e-5 * scale):
            fails.append(f"{name}: {err:.3e} of {scale:.3e}")
    # the reference side: full ref_q and one 16-channel block of it
    src_vals = {l: (st[l] if st is not None else fg[l].detach()) for l in (1, 2, 3)}
    for name, sl in (("ref_q full", slice(0, 96)), ("ref_q block 48..63", slice(48, 64))):
        d = torch.zeros((b, h, w, 96), device=DEV)
        d[..., sl] = torch.randn((b, h, w, sl.stop - sl.start), device=DEV)
        rhs = float((rq.grad.double() * d.double()).sum())
        err, scale = _identity(fwd(src_vals, d), rhs)
        worst = max(worst, err / max(scale, 1e-300))
        if not (scale > 0 and err <= 1e-5 * scale):
            fails.append(f"{name}: {err:.3e} of {scale:.3e}")
    print(f"iteration adjoint identities {size} {storage}: worst {worst:.2e} (bound 1e-5)")
    assert not fails, fails


@gpu
@pytest.mark.parametrize("storage", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("size", ["cfg4", "cfg5"])
def test_corr_init_backward_adjoint_identity(size, storage):
    b, v, ih, iw = ADJ_SIZES[size]
    h3, w3 = ih // 8, iw // 8
    p12_3 = _cams(b, v, ih, iw)[2]
    torch.manual_seed(4)
    dt = STORAGE[storage]
    fg = torch.randn((b * v, 48, h3, w3), device=DEV).contiguous(memory_format=CL).requires_grad_(True)
    st = None if dt is None else fg.detach().to(dt)
    inv_min, inv_max = torch.full((b,), 1 / 425.0, device=DEV), torch.full((b,), 1 / 935.0, device=DEV)
    proj = cu(p12_3)
    gout = torch.randn((b, v - 1, 32, 8, h3, w3), device=DEV)
    out = ops().corr_init_train(fg, b, v, proj, inv_min, inv_max, 32, stored=st)
    (out * gout).sum().backward()
    grad = fg.grad.view(b, v, 48, h3, w3)
    vals = (st if st is not None else fg.detach()).view(b, v, 48, h3, w3)

    def fwd(f):
        with torch.no_grad():
            f = f.reshape(b * v, 48, h3, w3).contiguous(memory_format=CL)
            o = ops().corr_init_train(f.float(), b, v, proj, inv_min, inv_max, 32, stored=f if dt is not None else None)
        return (o.double() * gout.double()).reshape(-1)

    fails, worst = [], 0.0
    for name, mask in _probes(fg.shape, b, v).items():
        d = torch.randn((b, v, 48, h3, w3), device=DEV) * mask
        d = d.to(dt) if dt is not None else d
        f = vals.clone()
        f[:, 1:] = d[:, 1:]                                           # sources = the probe, reference view as stored
        rhs = float((grad[:, 1:].double() * d[:, 1:].double()).sum())
        err, scale = _identity(fwd(f), rhs)
        worst = max(worst, err / max(scale, 1e-300))
        if not (scale > 0 and err <= 1e-5 * scale):
            fails.append(f"{name}: {err:.3e} of {scale:.3e}")
    for name, sl in (("reference view full", slice(0, 48)), ("reference view block 16..31", slice(16, 32))):
        d = torch.zeros((b, 48, h3, w3), device=DEV)
        d[:, sl] = torch.randn((b, sl.stop - sl.start, h3, w3), device=DEV)
        d = d.to(dt) if dt is not None else d
        f = vals.clone()
        f[:, 0] = d
        rhs = float((grad[:, 0].double() * d.double()).sum())
        err, scale = _identity(fwd(f), rhs)
        worst = max(worst, err / max(scale, 1e-300))
        if not (scale > 0 and err <= 1e-5 * scale):
            fails.append(f"{name}: {err:.3e} of {scale:.3e}")
    print(f"initialisation adjoint identities {size} {storage}: worst {worst:.2e} (bound 1e-5)")
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------
# FeatureGradPool: one initialisation + four iteration calls of a training step into shared accumulators
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_pooled_feature_gradients_equal_the_separate_calls_and_fp64():
    from itermvs_amd.engine import sample_offsets
    storage, b, s = "fp16", 2, 4
    c = _iter_inputs(s, b, True, False, seed=77)
    v = c["v"]
    feats = {l: stored_values(f, storage) for l, f in c["feats"].items()}
    c["feats"] = feats
    gen = torch.Generator().manual_seed(78)
    h, w = c["h"], c["w"]
    calls = [dict(nd=torch.rand((b, 1, h, w), generator=gen), vw=torch.rand((b, s, h, w), generator=gen),
                  ref_q=torch.randn((b, h, w, 96), generator=gen),
                  gout=[torch.randn((b, NHYP[l], 8, h, w), generator=gen) for l in (1, 2, 3)]) for _ in range(4)]
    h3, w3 = c["sizes"][3]
    g_init = torch.randn((b, s, 32, 8, h3, w3), generator=gen)
    p12 = c["p12"]
    inv_min, inv_max = c["inv_min"], c["inv_max"]
    dt = STORAGE[storage]

    def run(pooled):
        base = {l: cu(feats[l]).contiguous(memory_format=CL).requires_grad_(True) for l in (1, 2, 3)}
        pool = ops().FeatureGradPool() if pooled else None
        legs = []
        if pooled:
            fd = ops().feature_grad_sink(pool, base)
            legs = [fd] * 5
        else:
            legs = [{l: cu(feats[l]).contiguous(memory_format=CL).requires_grad_(True) for l in (1, 2, 3)} for _ in range(5)]
        st = [{l: legs[k][l].detach().to(dt) for l in (1, 2, 3)} for k in range(5)]
        loss = (ops().corr_init_train(legs[0][3], b, v, cu(p12[2]), cu(inv_min), cu(inv_max), 32, stored=st[0][3], pool=pool)
                * cu(g_init)).sum()
        rqs = []
        for k, cl in enumerate(calls):
            rq = cu(cl["ref_q"]).requires_grad_(True)
            rqs.append(rq)
            outs = ops().corr_iter_train(legs[k + 1], b, v, rq, cu(p12), cu(cl["vw"]), cu(inv_min), cu(inv_max), cu(cl["nd"]),
                                         sample_offsets(), stored=st[k + 1], pool=pool)
            loss = loss + sum((o * cu(g)).sum() for o, g in zip(outs, cl["gout"]))
        loss.backward()
        if pooled:
            grads = {l: base[l].grad.cpu() for l in (1, 2, 3)}
        else:
            grads = {l: sum(legs[k][l].grad.cpu() for k in range(5) if legs[k][l].grad is not None) for l in (1, 2, 3)}
        return grads, [rq.grad.cpu() for rq in rqs]

    pooled, rq_p = run(True)
    single, rq_s = run(False)
    # the fp64 reference: one initialisation (level 3) + four iteration calls
    want = {l: torch.zeros_like(feats[l], dtype=torch.float64) for l in (1, 2, 3)}
    depth0 = O.initial_depth_samples(inv_min.view(b, 1, 1, 1), inv_max.view(b, 1, 1, 1), h3, w3)
    want[3] += R.corr_init_grads(feats[3], p12[2], depth0, g_init, b, v)
    want_rq = []
    for cl in calls:
        depth = O.iteration_depth_samples(cl["nd"], inv_min.view(b, 1, 1, 1), inv_max.view(b, 1, 1, 1))
        gf, grq = R.corr_iter_grads(feats, cl["ref_q"], p12, cl["vw"], depth, cl["gout"], b, v)
        for l in (1, 2, 3):
            want[l] += gf[l]
        want_rq.append(grq)
    ok = True
    for l in (1, 2, 3):
        ok &= report(f"pooled vs separate calls, level {l}", *R.parity(pooled[l], single[l]), 1e-6)
        ok &= report(f"pooled vs fp64, level {l}", *R.parity(pooled[l], want[l]))
    for k in range(4):
        assert torch.equal(rq_p[k], rq_s[k])                         # dL/dref_q: written once per call, never pooled
        ok &= report(f"dL/dref_q call {k} vs fp64", *R.parity(rq_p[k], want_rq[k]))
    assert ok
