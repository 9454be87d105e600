"""The deferred NaN-projection assert (module.py:83,87) at kernel and forward level.

The reference asserts ``not torch.isnan(src_proj @ torch.inverse(ref_proj)).any()`` before it changes any weight.  Here the
camera composition (``itermvs_compose_proj`` and its two fused launches, ``itermvs_ref_quarter_compose`` and
``itermvs_stem_compose``) ORs a device flag instead, and the training step / engine raise afterwards.  The kernel's decision is
"some element of the 3x4 rows of src @ inverse(ref) is NaN", with the inverse formed in fp64 by Gauss-Jordan elimination with
partial pivoting (itermvs_amd/csrc/compose.hpp).  ``_kernel_rule`` restates that elimination in Python floats (IEEE fp64, the
kernels are built with -ffp-contract=off), ``_reference_rule`` is the reference's fp32 rule on the CPU (a ``torch.inverse``
that raises on a singular matrix counts as flagged).

The camera table holds well-conditioned rigs, exactly singular and non-finite cameras, and a near-singular band where the
fp32 and fp64 decisions may differ: condition numbers from 1e7 up, and matrices singular in exact arithmetic whose
elimination leaves a rounding residue instead of a zero pivot.  For the band the kernel's documented fp64 rule is
asserted and the fp32 reference's decision printed next to it."""
import math

import numpy as np
import pytest
import torch

from conftest import load_weights

DEV = "cuda"
NAN, INF = float("nan"), float("inf")


def ops():
    from itermvs_amd import ops as _ops
    return _ops


# ---- the two decision rules, on the CPU ----------------------------------------------------------------------------------
def _kernel_compose(ref: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """compose_proj_body in Python floats: the fp64 Gauss-Jordan inverse of ``ref`` in the kernel's order, the 3x4 rows of
    src @ inverse(ref) accumulated over k = 0..3 in fp64 and rounded once to fp32."""
    a = [[float(ref[i, j]) for j in range(4)] + [1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for c in range(4):
        piv, best = c, abs(a[c][c])
        for r in range(c + 1, 4):
            if abs(a[r][c]) > best:
                best, piv = abs(a[r][c]), r
        a[c], a[piv] = a[piv], a[c]
        p = a[c][c]
        inv = (math.copysign(INF, p) if p == 0.0 else 1.0 / p) if p == p else NAN    # IEEE 1/x, which Python refuses for 0
        a[c] = [x * inv for x in a[c]]
        for r in range(4):
            if r != c:
                f = a[r][c]
                a[r] = [a[r][j] - f * a[c][j] for j in range(8)]
    out = torch.empty(12, dtype=torch.float32)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(4):
                acc = 0.0
                for k in range(4):
                    acc += float(src[i, k]) * a[k][4 + j]
                out[i * 4 + j] = float(np.float32(acc))
    return out


def _kernel_rule(mats: torch.Tensor) -> bool:
    return any(bool(torch.isnan(_kernel_compose(m[0], m[s])).any()) for m in mats for s in range(1, m.shape[0]))


def _reference_rule(mats: torch.Tensor) -> bool:
    """models/module.py:86-87 in fp32 on the CPU, per (set, source view)"""
    for m in mats:
        try:
            inv = torch.inverse(m[0])
        except RuntimeError:                          # torch.linalg.LinAlgError: an exactly singular pivot
            return True
        for s in range(1, m.shape[0]):
            if bool(torch.isnan(m[s] @ inv).any()):
                return True
    return False


# ---- the camera table ----------------------------------------------------------------------------------------------------
def _rig(batch, views, height, width, seed):
    """the pipeline's form: [3 * B, V, 4, 4], set = level * B + item (levels 1, 2, 3)"""
    from itermvs_amd import synthetic
    pm = synthetic.make_sample(batch, views, height, width, seed=seed)["proj_matrices"]
    return torch.cat([pm[f"level_{l}"].float() for l in (1, 2, 3)]).contiguous()


# a camera whose Gauss-Jordan steps are exact in fp32 and fp64 (pivots and their ratios powers of two), so that a duplicated or
# summed row leaves an exactly zero pivot under both rules
P2 = torch.tensor([[256.0, 0.0, 64.0, 1024.0], [0.0, 256.0, 48.0, 2048.0], [0.0, 0.0, 1.0, 512.0], [0.0, 0.0, 0.0, 1.0]])


def _near_singular(sigma: float, seed: int) -> torch.Tensor:
    """U diag(1, 1, 1, sigma) V^T rounded to fp32: a reference camera of condition number ~1 / sigma"""
    gen = torch.Generator().manual_seed(seed)
    u, _ = torch.linalg.qr(torch.randn((4, 4), generator=gen, dtype=torch.float64))
    v, _ = torch.linalg.qr(torch.randn((4, 4), generator=gen, dtype=torch.float64))
    return (u @ torch.diag(torch.tensor([1.0, 1.0, 1.0, sigma], dtype=torch.float64)) @ v.T).float()


def camera_table():
    """[(name, mats [n_sets, V, 4, 4] fp32, band)]; ``band``: near-singular, the fp32 and fp64 rules may decide differently"""
    base = _rig(2, 3, 96, 128, seed=3)                                   # B = 2, 3 views, sets (level 1..3) x (item 0, 1)
    t = [("rig_b2", base, False), ("cfg1", _rig(1, 5, 512, 640, seed=0), False), ("cfg5", _rig(1, 11, 1280, 1920, seed=1), False)]

    def edit(name, fn, band=False):
        m = base.clone()
        fn(m)
        t.append((name, m, band))

    def p2_ref(rows):
        def fn(m):
            r = P2.clone()
            rows(r)
            m[0, 0] = r
        return fn

    edit("ref_zero_row", lambda m: m[0, 0, 1].zero_())
    edit("ref_dup_row", p2_ref(lambda r: r[2].copy_(r[0])))
    edit("ref_rank3", p2_ref(lambda r: r[2].copy_(r[0] + r[1])))
    edit("ref_nan", lambda m: m[0, 0, 1].__setitem__(2, NAN))
    edit("src_nan_one_view", lambda m: m[0, 2, 0].__setitem__(3, NAN))
    edit("src_nan_third_row", lambda m: m[0, 1, 2].__setitem__(1, NAN))       # only output row 2 is NaN
    edit("ref_pos_inf", lambda m: m[0, 0, 0].__setitem__(0, INF))
    edit("ref_neg_inf", lambda m: m[0, 0, 2].__setitem__(3, -INF))
    edit("src_pos_inf_translation", lambda m: m[0, 1, 1].__setitem__(3, INF))  # meets inverse(ref)[3, 0] == 0: inf * 0
    edit("src_neg_inf_translation", lambda m: m[0, 2, 0].__setitem__(3, -INF))
    edit("src_pos_inf_rotation", lambda m: m[0, 1, 0].__setitem__(2, INF))     # only non-zero factors: +-inf, no NaN
    edit("src_neg_inf_rotation", lambda m: m[0, 2, 2].__setitem__(2, -INF))
    edit("item1_only", lambda m: [m[s, 0, 1].zero_() for s in (1, 3, 5)])   # every level of batch item 1, item 0 clean
    edit("level3_only", lambda m: [m[s, 1, 2].__setitem__(0, NAN) for s in (4, 5)])   # level 3 of both items, levels 1, 2 clean
    # the band: rounding decides whether a pivot is exactly zero (camera rows duplicated / summed in fp32, whose elimination
    # leaves a rounding residue), or the matrix is merely ill-conditioned
    # inverse(ref)[1, 0] is 0 in exact arithmetic: fp32 LAPACK returns 0 (inf * 0 = NaN), the fp64 elimination a residue of
    # 1.8e-12 (inf * 1.8e-12 = inf)
    edit("band_src_inf_times_rounded_zero", lambda m: m[0, 1, 1].__setitem__(1, INF), band=True)
    edit("band_cam_dup_row", lambda m: m[0, 0, 2].copy_(m[0, 0, 0]), band=True)
    edit("band_cam_rank3", lambda m: m[0, 0, 2].copy_(m[0, 0, 0] + m[0, 0, 1]), band=True)
    third = float(np.float32(1.0 / 3.0))
    edit("band_fp32_third", lambda m: m[0, 0].copy_(torch.tensor([[3.0, 1.0, 0.0, 0.0], [1.0, third, 0.0, 1.0],
                                                                  [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])), band=True)
    for k, sigma in enumerate((1e-7, 1e-8, 1e-9)):
        edit(f"band_sigma_{sigma:.0e}", lambda m, s=sigma, k=k: m[0, 0].copy_(_near_singular(s, k)), band=True)
    return t


def _depth_range(n):
    return torch.linspace(425.0, 450.0, n), torch.linspace(900.0, 935.0, n)


def test_camera_table_decisions_on_the_cpu():
    """the table itself: a well-posed entry is decided alike by the reference's fp32 rule and the kernel's fp64 rule, and the
    entries that must flag do; the band entries are ill-conditioned (measured in fp64) -- their decisions are reported"""
    must_flag = {"ref_zero_row", "ref_dup_row", "ref_rank3", "ref_nan", "src_nan_one_view", "src_nan_third_row", "ref_neg_inf",
                 "src_pos_inf_translation", "src_neg_inf_translation", "item1_only", "level3_only"}
    for name, mats, band in camera_table():
        k, r = _kernel_rule(mats), _reference_rule(mats)
        if band:
            cond = float(torch.linalg.cond(mats[0, 0].double()))
            print(f"{name}: condition {cond:.2e}; fp64 kernel rule {int(k)}, fp32 reference rule {int(r)}")
            assert cond >= 1e6, (name, cond)
        else:
            assert k == r == (name in must_flag), (name, k, r)
    # the third-row case is flagged only through output row 2
    m = dict((n, x) for n, x, _ in camera_table())["src_nan_third_row"]
    out = _kernel_compose(m[0, 0], m[0, 1]).view(3, 4)
    assert not bool(torch.isnan(out[:2]).any()) and bool(torch.isnan(out[2]).any())


# ---- A: the flag kernel --------------------------------------------------------------------------------------------------
def _launch(form, mats, flag, dmin, dmax):
    """one launch of the composition in ``form``; returns (proj, inv_min, inv_max)"""
    mats, dmin, dmax = mats.to(DEV), dmin.to(DEV), dmax.to(DEV)
    if form == "compose_proj":
        return ops().compose_proj(mats, flag, (dmin, dmax))
    if form == "ref_quarter_compose":
        gen = torch.Generator().manual_seed(2)
        b, h, w = 2, 12, 16
        cl = lambda *s: torch.randn(s, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last)  # noqa: E731
        _, proj, imin, imax = ops().ref_quarter_compose(cl(b, 16, 2 * h, 2 * w), cl(b, 32, h, w), cl(b, 48, h // 2, w // 2), mats,
                                                        flag, (dmin, dmax))
        return proj, imin, imax
    x = torch.randn((2, 3, 34, 46), generator=torch.Generator().manual_seed(3)).to(DEV)
    _, _, proj, imin, imax = ops().stem(x, *_stem_weights(), compose=(mats, flag, (dmin, dmax)))
    return proj, imin, imax


_SW = []


def _stem_weights():
    if not _SW:
        from itermvs_amd.engine import fold_batchnorm
        wts = {k: v.to(DEV) for k, v in load_weights("dtu").items() if k.startswith("feature_net.")}
        _SW.extend(ops().pack_stem_weights(*[t for n in ("conv1.", "layer1.0.conv1.", "layer1.0.downsample.")
                                             for t in fold_batchnorm(wts, "feature_net." + n)]))
    return _SW


FORMS = ["compose_proj", "ref_quarter_compose", "stem"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_nan_flag_against_the_reference_decision(form):
    """For every camera set of the table, in ``form``: the flag is set exactly when the rule says so; a flagged set's finite
    outputs equal those of each of its sets launched alone and those of the kernel's elimination restated on the CPU, bit for
    bit; the flag is OR-only
    (a clean launch after a flagged one leaves it at 1); finite outputs match the fp64 composition like
    test_compose_proj_matches_fp64_and_reference (1e-6 element-wise; the band: 1e-6 of the largest element)."""
    table = camera_table()
    clean = table[0][1]
    report = []
    for name, mats, band in table:
        want = _kernel_rule(mats)
        ref32 = _reference_rule(mats)
        if not band:
            assert want == ref32, (name, want, ref32)
        n, v = mats.shape[:2]
        dmin, dmax = _depth_range(n)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        proj, imin, imax = (t.cpu() for t in _launch(form, mats, flag, dmin, dmax))
        got = bool(flag.item())
        assert got == want, (form, name, got, want)
        if band:
            report.append(f"{name}: kernel {int(got)} (fp64 rule {int(want)}), fp32 reference {int(ref32)}")
        assert torch.equal(imin, 1.0 / dmin) and torch.equal(imax, 1.0 / dmax), name
        # OR-only: a clean launch leaves a raised flag raised
        _launch(form, clean, flag, *_depth_range(clean.shape[0]))
        assert int(flag.item()) == int(want), (form, name)
        # the same sets launched one at a time: same bits (NaN where NaN), and the flag of the set that carries the fault
        for i in range(n):
            f1 = torch.zeros(1, dtype=torch.int32, device=DEV)
            alone = ops().compose_proj(mats[i:i + 1].to(DEV), f1).cpu()
            torch.testing.assert_close(proj[i:i + 1], alone, rtol=0, atol=0, equal_nan=True)
            assert bool(f1.item()) == _kernel_rule(mats[i:i + 1]), (name, i)
        # the kernel's elimination restated in Python floats (IEEE fp64, no contraction): the same bits, NaN where NaN
        for i in range(n):
            for s in range(1, v):
                mirror = _kernel_compose(mats[i, 0], mats[i, s])
                torch.testing.assert_close(proj[i, s - 1], mirror, rtol=0, atol=0, equal_nan=True, msg=f"{form} {name} {i} {s}")
        # finite outputs against the fp64 composition, for every set with an invertible finite reference
        for i in range(n):
            ref = mats[i, 0].double()
            if not bool(torch.isfinite(ref).all()) or float(torch.linalg.cond(ref)) > 1e12:
                continue
            inv = torch.inverse(ref)
            for s in range(1, v):
                exact = (mats[i, s].double() @ inv)[:3, :4].reshape(12)
                g = proj[i, s - 1].double()
                ok = torch.isfinite(exact)
                assert torch.equal(torch.isfinite(g), ok), (name, i, s, g, exact)
                if not bool(ok.any()):
                    continue
                g, exact = (torch.where(ok, t, torch.zeros_like(t)) for t in (g, exact))     # finite elements only
                if band:
                    err = float((g - exact).abs().max()) / float(exact.abs().max())
                else:
                    err = float(((g - exact).abs() / exact.abs().clamp(min=1e-3)).max())
                assert err < 1e-6, (form, name, i, s, err)
    print(f"{form}: near-singular band: " + "; ".join(report))


@pytest.mark.gpu
def test_nan_flag_launch_forms_agree_bit_for_bit():
    """the whole table concatenated into one launch per view count, in each of the three forms: the same bits as compose_proj
    of each entry alone, and the flag is the OR of the entries'"""
    by_views = {}
    for name, mats, _ in camera_table():
        by_views.setdefault(mats.shape[1], []).append(mats)
    for v, parts in by_views.items():
        mats = torch.cat(parts)
        dmin, dmax = _depth_range(mats.shape[0])
        want = [ops().compose_proj(p.to(DEV)).cpu() for p in parts]
        for form in FORMS:
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            proj, _, _ = _launch(form, mats, flag, dmin, dmax)
            torch.testing.assert_close(proj.cpu(), torch.cat(want), rtol=0, atol=0, equal_nan=True)
            assert bool(flag.item()) == _kernel_rule(mats), (form, v)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_depth_range_edges_do_not_flag(form):
    """a zero or negative depth_min is not a camera fault (the reference asserts on the projection only): 1 / depth_min is what
    IEEE division gives (+inf, -inf, a negative number) and the flag stays clear"""
    mats = _rig(2, 3, 96, 128, seed=3)[:4]
    dmin = torch.tensor([0.0, -0.0, -2.0, 425.0])
    dmax = torch.tensor([935.0, -0.0, -3.0, 0.0])
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    _, imin, imax = _launch(form, mats, flag, dmin, dmax)
    assert int(flag.item()) == 0
    imin, imax = imin.cpu(), imax.cpu()
    assert torch.equal(imin, 1.0 / dmin) and torch.equal(imax, 1.0 / dmax)
    assert imin[0] == INF and imin[1] == -INF and imin[2] == -0.5 and imax[3] == INF


# ---- B: the training forward with a bad camera ---------------------------------------------------------------------------
def _bad_batch(kind):
    """the 96x128, B = 2, 3-view training batch with a bad camera: ``singular`` = item 0's reference camera zeroed at every
    level; ``src_nan`` = one NaN in source view 2 of item 1 at every level"""
    from itermvs_amd import synthetic
    imgs, projs, dmin, dmax, gt, mask = synthetic.make_training_batch(2, num_views=3, height=96, width=128, seed=70, hole_fraction=0.1)
    projs = {k: v.clone() for k, v in projs.items()}
    for k in projs:
        if kind == "singular":
            projs[k][0, 0] = 0.0
        elif kind == "src_nan":
            projs[k][1, 2, 1, 2] = NAN
    to = lambda d: {k: v.to(DEV) for k, v in d.items()}  # noqa: E731
    return to(imgs), to(projs), dmin.to(DEV), dmax.to(DEV), to(gt), to(mask)


def _model():
    from itermvs_amd.net import Pipeline
    m = Pipeline(iteration=2, test=False)
    m.load_state_dict(load_weights("seed0"))
    return m.to(DEV).train()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["singular", "src_nan"])
def test_training_forward_with_a_bad_camera(kind):
    """Eager (no deferral): the assert fires after the forward, before anything is updated -- parameters and Adam's state are
    unchanged.  Deferred (``train_nan_flag`` set, CapturedTrainStep's mode): the forward completes, every output has its shape
    and the flag is raised.  The bad camera really reaches the computation: the batch item it belongs to comes out different
    from the same batch with good cameras.  Nothing non-finite leaks out of the correlation kernels, though: a NaN
    projection puts every tap at a non-finite (or behind-camera) coordinate, whose bilinear weights are zero
    (common.hpp make_taps / project_fast), so loss and outputs stay finite -- which is why the training step must skip a
    flagged step explicitly rather than rely on NaN gradients.  FeatureNet's BatchNorm running statistics move, as they do
    in the reference, whose assert fires inside the warp AFTER FeatureNet ran."""
    from itermvs_amd.net import full_loss
    imgs, projs, dmin, dmax, gt, mask = _bad_batch(kind)
    model = _model()
    opt = torch.optim.Adam(model.parameters(), lr=1e-5)
    good = _bad_batch("none")
    opt.zero_grad(set_to_none=True)
    out = model(*good[:4])
    full_loss(out["depths"], out["depths_upsampled"], out["confidences"], good[4], good[5], good[2], good[3], True).backward()
    opt.step()                                                               # Adam state exists
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    state = {k: {n: (v.clone() if torch.is_tensor(v) else v) for n, v in st.items()} for k, st in opt.state.items()}
    rm = model.state_dict()["feature_net.conv1.bn.running_mean"].clone()
    opt.zero_grad(set_to_none=True)
    with pytest.raises(AssertionError, match="nan in proj"):
        model(imgs, projs, dmin, dmax)
    for n, p in model.named_parameters():
        assert torch.equal(p, params[n]) and p.grad is None, n
    for k, st in opt.state.items():
        for n, val in st.items():
            assert torch.equal(val, state[k][n]) if torch.is_tensor(val) else val == state[k][n], n
    assert not torch.equal(model.state_dict()["feature_net.conv1.bn.running_mean"], rm)    # BatchNorm statistics moved

    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    model.train_nan_flag = flag
    with torch.no_grad():
        clean = model(*good[:4])
        out2 = model(imgs, projs, dmin, dmax)
    assert int(flag.item()) == 1
    for key in out["depths"]:
        assert [t.shape for t in out2["depths"][key]] == [t.shape for t in out["depths"][key]], key
    assert [t.shape for t in out2["confidences"]] == [t.shape for t in out["confidences"]]
    assert out2["depths_upsampled"][0].shape == out["depths_upsampled"][0].shape
    assert out2["confidence_upsampled"].shape == out["confidence_upsampled"].shape
    item = 0 if kind == "singular" else 1
    assert not torch.equal(out2["depths_upsampled"][0][item], clean["depths_upsampled"][0][item])
    loss = full_loss(out2["depths"], out2["depths_upsampled"], out2["confidences"], gt, mask, dmin, dmax, True)
    print(f"{kind}: deferred forward loss {float(loss):.6f}")
    assert math.isfinite(float(loss)) and bool(torch.isfinite(out2["depths_upsampled"][0]).all())
    assert all(bool(torch.isfinite(b).all()) for n, b in model.named_buffers() if "running" in n)
