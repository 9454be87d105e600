"""Chaos-free full-size parity: every HIP stage of the engine is fed the CPU oracle's OWN inputs for that stage
(teacher forcing), so a deviation never feeds back through the arg-max / GRU and the tolerances can be the kernels'
real ones instead of a platform-floor ratio.

For the init stage and each of the GRU iterations (models/itermvs.py:270-324) the oracle's trace provides the stage
inputs; the engine's stage methods (itermvs_amd/engine.py: stage_init / stage_score0 / stage_hidden0 / stage_head /
stage_corr / stage_corrnets / stage_gru / confidence / convex up-sampling) run on them and are compared with the
oracle's stage outputs:

    aggregated correlations (CorrNet inputs)   <= 5e-5 * scale
    CorrNet scores, hidden states, confidence  <= 1e-4 * scale
    arg-max bins                               IDENTICAL wherever the oracle's top-2 logit gap > 1e-4 * max(1, |top logit|)
                                               (>= 99 % of the pixels in every case)
    normalised depth                           <= 1e-4 there
    up-sampled depth / confidence              <= 1e-5 relative / 1e-6

scale = max(1, max |oracle tensor|).  Cases: BASELINE cfg 1 with the published DTU weights (photo-consistent scene and
noise images), the cfg-3 shape (5 views, 1600x1152) with the seeded weights, the cfg-5 geometry, and the routes those
miss: B = 2 with a different rig and depth range per item, one and two source views, grids that end in a partial tile
of every tiled kernel (224x352: 28x44 at 1/8, 56x88 at 1/4), a grid smaller than any tile (32x64), bf16 storage.
Every case runs in both convolution arithmetics (``conv_arithmetic`` "bf16x3" and "fp32": different kernels for
FeatureNet, the stem, the initial correlation layout, CorrNet, the heads and the ConvGRU); the bf16x3 runs also check
the ConvGRU's layer-by-layer form (``gru_coop = False``, what maps above 3.1 M pixels run).
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_weights
from oracle import itermvs_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
HID = 32


def cu(t):
    return t.to(DEV)


def rel_err(got, want):
    """max |got - want| / max(1, max |want|)"""
    want = want.detach().cpu().float()
    return float((got.detach().cpu().float() - want).abs().max()) / max(1.0, float(want.abs().max()))


FAILS = []


def need(cond, msg):
    """deferred assert: every stage is measured before the test fails, the report lists all deviations"""
    if not cond:
        FAILS.append(msg)


def check_head(eng, ws, w_cpu, hidden_o, best_o, nd_o, tag):
    """depth head + regression on the oracle's hidden state, fused launch and layer-by-layer form; the decided fraction
    and the arg-max flips per batch item"""
    logits_o = O.depth_head_logits(w_cpu, hidden_o)
    top2 = torch.topk(logits_o, 2, dim=1).values
    # the oracle's own arg-max is not a near-tie: top-2 gap > 1e-4 relative to the winning logit (>= 1e-4 absolute)
    decided = (top2[:, :1] - top2[:, 1:2]) > 1e-4 * top2[:, :1].abs().clamp(min=1.0)
    frac = [float(decided[i].float().mean()) for i in range(decided.shape[0])]
    for i, f in enumerate(frac):
        need(f >= 0.99, f"{tag}: only {f:.4f} decided pixels in item {i}")
    out = {}
    for form in ("fused", "layers"):
        ws["hidden"].copy_(cu(hidden_o))
        logits, best = eng.stage_head(ws, want_logits=(form == "layers"), want_best=True)
        best = best.cpu()
        nd = ws["hx"][:, HID:HID + 1].cpu()
        need(torch.equal(ws["hx2"][:, HID:HID + 1].cpu(), nd), f"{tag}/{form}: hx2 depth channel differs")   # both GRU input buffers receive it
        flips = (best != best_o) & decided
        for i in range(flips.shape[0]):
            need(int(flips[i].sum()) == 0, f"{tag}/{form}: {int(flips[i].sum())} arg-max flips at decided pixels of item {i}")
        err = float(((nd - nd_o).abs() * decided).max())
        need(err <= 1e-4, f"{tag}/{form}: normalised depth off by {err:.2e}")
        if logits is not None:
            need(rel_err(logits, logits_o) <= 1e-4, f"{tag}: logits {rel_err(logits, logits_o):.2e}")
        out[form] = (float((best != best_o).float().mean()), err)
    return out, min(frac)


# (name, weights, inputs, batch seeds, views, height, width, iterations, feature storage)
# cfg5geom: BASELINE cfg 5's geometry (10 source views, 8 GRU iterations) on a 512x384 crop, fp32 and with the fp16
# feature storage that configuration names (the oracle models the storage: features rounded to fp16 before the matching
# stages, ``feature_storage``); the full 1920x1280 size is covered by test_full_size_configs_cross_backend.
# b2: two scenes with their own rigs, item 1 with its own depth range (B > 1: packed CorrNet scores, per-item strides,
# depth ranges and projections).  s1 / s2: one / two source views (the view weights' normalisation at its edge) on
# 224x352, whose 1/8 and 1/4 grids end in a partial tile of CorrNet (32x32), lat_conv (8x32) and the 16-column kernels.
# tiny: 32x64, the smallest size Pipeline accepts -- 4x8 at 1/8, smaller than any tile.
CASES = [
    ("cfg1-dtu-scene", "dtu", "scene", (0,), 5, 512, 640, 4, "fp32"),
    ("cfg1-dtu-noise", "dtu", "noise", (0,), 5, 512, 640, 4, "fp32"),
    ("cfg3-seed0-noise", "seed0", "noise", (0,), 5, 1152, 1600, 4, "fp32"),
    ("cfg5geom-dtu-scene", "dtu", "scene", (0,), 11, 384, 512, 8, "fp32"),
    ("cfg5geom-dtu-scene-fp16", "dtu", "scene", (0,), 11, 384, 512, 8, "fp16"),
    ("b2-dtu-scene", "dtu", "scene", (0, 1), 5, 256, 320, 4, "fp32"),
    ("s1-ragged-dtu-scene", "dtu", "scene", (0,), 2, 224, 352, 4, "fp32"),
    ("s2-ragged-dtu-scene-bf16", "dtu", "scene", (0,), 3, 224, 352, 2, "bf16"),
    ("b2-tiny-dtu-scene", "dtu", "scene", (0, 1), 3, 32, 64, 2, "fp32"),
]
# the depth range of item 1 of the B = 2 cases differs from item 0's (DTU: 425..935)
DEPTH_RANGES = {"b2-dtu-scene": ((425.0, 935.0), (380.0, 1000.0)), "b2-tiny-dtu-scene": ((425.0, 935.0), (380.0, 1000.0))}
STORAGE = {"fp32": None, "fp16": torch.float16, "bf16": torch.bfloat16}
ARITHMETIC = ("bf16x3", "fp32")
# (the bf16x3 items keep the ids they had before the arithmetic became a parameter; the two forms of a case run back to back)
PARAMS = [pytest.param(c, a, id=c[0] if a == "bf16x3" else f"{c[0]}-fp32") for c in CASES for a in ARITHMETIC]

_ORACLE = {}


def oracle_case(case):
    """(sample, weights, oracle outputs, trace) of a case; the oracle does not depend on the engine's arithmetic, so the
    last case's run is kept (one entry: the cfg-3 trace alone is several GB) and the second arithmetic reuses it"""
    if case not in _ORACLE:
        _ORACLE.clear()
        name, wtag, kind, seeds, views, height, width, iters, storage = case
        from itermvs_amd import synthetic
        w_cpu = load_weights(wtag)
        if kind == "scene":
            s = synthetic.make_scene_batch(views, height, width, seeds, DEPTH_RANGES.get(name))
        else:
            assert len(seeds) == 1
            s = synthetic.make_sample(batch=1, num_views=views, height=height, width=width, seed=seeds[0])
        t = {}
        with torch.no_grad():
            out_o = O.pipeline_forward(w_cpu, s["imgs"], s["proj_matrices"], s["depth_min"], s["depth_max"], iters, trace=t,
                                       feature_storage=STORAGE[storage])
        _ORACLE[case] = (s, w_cpu, out_o, t)
    return _ORACLE[case]


@pytest.mark.parametrize("case,arithmetic", PARAMS)
def test_every_stage_on_the_oracles_inputs(case, arithmetic):
    from itermvs_amd import ops
    from itermvs_amd.engine import InferenceEngine
    torch.set_num_threads(min(32, max(8, torch.get_num_threads())))
    name, wtag, kind, seeds, views, height, width, iters, storage = case
    s, w_cpu, out_o, t = oracle_case(case)
    eng = InferenceEngine({k: cu(v) for k, v in w_cpu.items()}, iters, storage, conv_arithmetic=arithmetic)
    assert eng.split3 == (arithmetic == "bf16x3") and eng.gru_coop == eng.split3
    b, v = len(seeds), views
    assert s["imgs"]["level_0"].shape[:2] == (b, v)
    sv = v - 1
    h, wd = height // 4, width // 4
    ws = eng._workspace(b, h, wd)
    hx, hx2 = ws["hx"], ws["hx2"]
    report = {}
    FAILS.clear()

    def lim(name, value, bound):
        report[name] = value
        need(value <= bound, f"{name} = {value:.2e} > {bound:.0e}")

    # FeatureNet on the same images (the only stage whose input is not an oracle intermediate)
    with torch.no_grad():
        feats = eng.feature_net(cu(s["imgs"]["level_0"]).reshape(b * v, 3, height, width).contiguous())
    # 16-bit storage: the engine's features are its fp32 results rounded once to nearest, which moves an element by at most
    # the unit roundoff times the power of two below it -- 2^-11 (fp16, 11 significant bits) / 2^-8 (bf16, 8 bits) of
    # max |want|; the oracle's unrounded features are the reference (bf16 at 224x352: 3.4e-3 measured from rounding alone)
    feat_lim = {"fp32": 2e-5, "fp16": 5e-4, "bf16": 4e-3}[storage]
    for l in (1, 2, 3):
        assert feats[l].dtype == (STORAGE[storage] or torch.float32)
        lim(f"feat{l}", rel_err(feats[l], t["feats"][l]), feat_lim)

    # stage inputs from the oracle: (stored) features, reference-faithful fp32 projections (module.py:77-90), depth range
    cl = {l: cu(t["feats_gathered"][l]).to(feats[l].dtype).contiguous(memory_format=torch.channels_last) for l in (1, 2, 3)}
    for l in (1, 2, 3):        # the oracle's rounded features are exactly representable in the storage type
        assert torch.equal(cl[l].float().cpu(), t["feats_gathered"][l])
    pv = {l: cl[l].view(b, v, *cl[l].shape[1:]) for l in (1, 2, 3)}
    src = {l: [pv[l][:, i] for i in range(1, v)] for l in (1, 2, 3)}
    ref = {l: pv[l][:, 0] for l in (1, 2, 3)}
    pm = [s["proj_matrices"][f"level_{l}"].float() for l in (1, 2, 3)]
    p12 = torch.stack([torch.stack([O.compose_projection(pm[i][:, k], pm[i][:, 0])[:, :3, :4].reshape(-1, 12)
                                    for k in range(1, v)], 1) for i in range(3)]).contiguous()      # [3,B,S,12]
    proj = cu(p12)
    inv_min, inv_max = cu(1.0 / s["depth_min"].float()), cu(1.0 / s["depth_max"].float())
    with torch.no_grad():
        ref_q = ops.ref_quarter(ref[1], ref[2], ref[3])

        # ---- initialisation (itermvs.py:270-276) ----
        tr = {}
        view_w = eng.stage_init(ws, src[3], ref[3], proj[2], inv_min, inv_max, trace=tr)
        lim("init.agg", rel_err(tr["init_agg"], t["init_agg"].permute(0, 2, 1, 3, 4)), 5e-5)
        lim("init.view_w", rel_err(view_w, t["view_weights"]), 1e-4)
        score0 = eng.stage_score0(cu(t["init_agg"].permute(0, 2, 1, 3, 4).contiguous()))
        lim("init.score", rel_err(score0, t["init_score"]), 1e-4)
        eng.stage_hidden0(ws, cu(t["init_score"]))
        lim("hidden0", rel_err(ws["hidden"], t["hidden0"]), 1e-4)
        need(torch.equal(hx[:, :HID], ws["hidden"]), "hidden0: the two copies differ")
        report["head0"], report["decided0"] = check_head(eng, ws, w_cpu, t["hidden0"], t["best0"], t["nd0"], "init")

        # ---- iterations (itermvs.py:288-324) ----
        hidden_in = t["hidden0"]
        view_w_o = cu(t["view_weights"])
        for it, ti in enumerate(t["iters"]):
            hx[:, :HID].copy_(cu(hidden_in))
            hx[:, HID:HID + 1].copy_(cu(ti["nd_in"]))
            hx2[:, HID:HID + 1].copy_(cu(ti["nd_in"]))
            aggs = eng.stage_corr(ws, src, ref_q, proj, view_w_o, inv_min, inv_max)
            for i, a in enumerate(aggs):
                want = ti["aggs"][i].permute(0, 2, 1, 3, 4)
                lim(f"it{it}.agg{i + 1}", rel_err(a, want), 5e-5)
                ws["agg"][i].copy_(cu(want))
            eng.stage_corrnets(ws)
            lim(f"it{it}.score", rel_err(hx[:, HID + 1:], ti["score"]), 1e-4)
            need(torch.equal(hx2[:, HID + 1:], hx[:, HID + 1:]), f"it{it}: score copies differ")
            hx[:, HID + 1:].copy_(cu(ti["score"]))
            hx2[:, HID + 1:].copy_(cu(ti["score"]))
            gru_in = (hx.clone(), hx2.clone())
            eng.stage_gru(ws)
            lim(f"it{it}.hidden", rel_err(ws["hidden"], ti["hidden"]), 1e-4)
            need(torch.equal(hx[:, :HID], ws["hidden"]), f"it{it}: hidden copies differ")
            if eng.gru_coop:
                # the form maps above 3.1 M pixels take (engine.stage_gru): conv2d with the fp32 z/r weights and the
                # bf16x3 q convolution, the gate math in their epilogues -- same inputs, same bounds
                hx.copy_(gru_in[0])
                hx2.copy_(gru_in[1])
                eng.gru_coop = False
                try:
                    eng.stage_gru(ws)
                finally:
                    eng.gru_coop = True
                lim(f"it{it}.hidden_conv2d", rel_err(ws["hidden"], ti["hidden"]), 1e-4)
                need(torch.equal(hx[:, :HID], ws["hidden"]), f"it{it}: hidden copies differ (conv2d form)")
            if ti["conf"] is not None:
                ws["hidden"].copy_(cu(ti["hidden"]))
                conf = eng.confidence(ws["hidden"], ws["conf"])
                lim("conf", rel_err(conf, ti["conf"]), 1e-4)
            report[f"it{it}.head"], _ = check_head(eng, ws, w_cpu, ti["hidden"], ti["best"], ti["nd"], f"iter {it}")
            hidden_in = ti["hidden"]

        # ---- final up-sampling (itermvs.py:262-264, 321-324) on the oracle's depth, logits and confidence ----
        last = t["iters"][-1]
        u = "iter_mvs.upsample."
        ref2 = t["feats"][2].view(b, v, *t["feats"][2].shape[1:])[:, 0]
        up_logits_o = F.conv2d(F.relu(F.conv2d(ref2, w_cpu[u + "0.weight"], padding=1)), w_cpu[u + "2.weight"])
        up_logits = eng.upsample_logits(cu(ref2).contiguous(), ws)
        lim("up_logits", rel_err(up_logits, up_logits_o), 1e-4)
        hx[:, HID:HID + 1].copy_(cu(last["nd"]))
        depth_up = ops.convex_upsample(cu(up_logits_o), hx, inv_min, inv_max, nd_channel=HID)
        d, d_o = depth_up.cpu(), out_o["depths_upsampled"]
        lim("depth_up", float(((d - d_o).abs() / d_o).max()), 1e-5)
        conf_up = ops.bilinear_up(cu(last["conf"]), 4)
        lim("conf_up", float((conf_up.cpu() - out_o["confidence_upsampled"]).abs().max()), 1e-6)
    print(f"teacher-forced {name} {arithmetic} B={b} V={v} {width}x{height}: " + ", ".join(
        f"{k}={v:.1e}" if isinstance(v, float) else f"{k}={v}" for k, v in report.items()))
    assert not FAILS, "; ".join(FAILS)


# ---------------------------------------------------------------------------------------------------------------------
# Teacher-forced BACKWARD at BASELINE cfg 4's size (round 4).  The training graph is chaotic end to end (an arg-max flip moves
# a regression window), so the end-to-end gradient gates of tests/test_train_gpu.py carry a measured chaos floor.  Here the
# fused correlation autograd Functions (the only hand-written backward on the path besides BatchNorm) are fed the pinned
# ORACLE's own tensors of a cfg-4 training step -- its FeatureNet pyramids (bf16-rounded for cfg 4 "as stated"), its view
# weights, its normalised depth going into a GRU iteration, and the UPSTREAM gradient dL/d(aggregated correlation) that the
# oracle's full_loss backward delivers to that Evaluation call -- and their input gradients are compared with torch autograd
# through the oracle's warp + group correlation + view-weighted mean on the same tensors.  Nothing feeds back: the
# tolerance is 1e-4 x scale at 640x512 with B = 2, like the 24x40 kernel tests.
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_corr_views(feat_pv, ref, p12_l, depth, size):
    """per-view group correlations [B,G,N,h,w] of one level: feat_pv [B,V,C,H1,W1], the oracle's differentiable pieces"""
    b, v = feat_pv.shape[:2]
    out = []
    for s in range(1, v):
        m = torch.cat([p12_l[:, s - 1].view(b, 3, 4), torch.zeros(b, 1, 4)], 1)
        with torch.no_grad():
            ix, iy, _ = O.warp_source_coords(m, depth, size[0], size[1])
        out.append(O.group_correlation(O.bilinear_gather(feat_pv[:, s], ix, iy), ref))
    return out


class _LazyTraces(dict):
    """storage name -> the traced oracle step with that feature storage, computed on first use (each storage's CPU oracle
    step is paid by the first test that needs it, not all of them by the first test of the module)"""

    def __init__(self, make):
        super().__init__()
        self._make = make

    def __missing__(self, name):
        self[name] = self._make(name)
        return self[name]


@pytest.fixture(scope="module")
def cfg4_backward_trace():
    """one cfg-4 shaped training step of the CPU oracle at B = 2 (5 views, 640x512, 4 iterations, seed-0 weights, the batch
    train.py --batch_size 2 builds), for fp32, bf16 and fp16 feature storage: traced tensors + the upstream gradients of
    every Evaluation call (retain_grad on the aggregated correlations)"""
    from itermvs_amd import synthetic
    torch.set_num_threads(min(32, max(8, torch.get_num_threads())))
    imgs, projs, dmin, dmax, gt, mk = synthetic.make_training_batch(2, num_views=5, height=512, width=640, seed=2, hole_fraction=0.1)

    def trace(name):
        storage = STORAGE[name]
        w = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in load_weights("seed0").items()}
        tr = {}
        res = O.pipeline_forward(w, imgs, projs, dmin, dmax, iteration=4, test=False, training=True, trace=tr, feature_storage=storage)
        for it in tr["iters"]:
            for a in it["aggs"]:
                a.retain_grad()
        O.full_loss(res["depths"], res["depths_upsampled"], res["confidences"], gt, mk, dmin, dmax, True).backward()
        return dict(
            feats={l: tr["feats_gathered"][l].detach() for l in (1, 2, 3)},
            view_w=tr["view_weights"].detach(),
            iters=[dict(nd_in=it["nd_in"].detach(), aggs=[a.detach() for a in it["aggs"]], up=[a.grad.detach() for a in it["aggs"]])
                   for it in tr["iters"]])

    out = _LazyTraces(trace)
    p = torch.stack([projs[f"level_{l}"] for l in (1, 2, 3)])
    p12 = torch.stack([torch.stack([O.compose_projection(p[i][:, s], p[i][:, 0])[:, :3, :4].reshape(-1, 12) for s in range(1, 5)], 1)
                       for i in range(3)])
    return out, p12, (1.0 / dmin), (1.0 / dmax)


@pytest.mark.parametrize("storage", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("it", [0, 2])
def test_corr_iter_backward_on_the_oracles_training_tensors(cfg4_backward_trace, storage, it):
    """itermvs_corr_iter_backward at 640x512, B = 2, 4 source views: dL/dsrc (scatter) and dL/dref_q (gather) for the
    oracle's upstream gradient of GRU iteration ``it`` (0: hypotheses around the first, noisy depth map; 2: a smooth one)"""
    from itermvs_amd import ops
    from itermvs_amd.engine import sample_offsets
    traces, p12, inv_min, inv_max = cfg4_backward_trace
    t = traces[storage]
    b, v = 2, 5
    feats = {l: t["feats"][l].clone().requires_grad_(True) for l in (1, 2, 3)}                  # [B*V,C,H,W], values as stored
    pv = {l: feats[l].view(b, v, *feats[l].shape[1:]) for l in (1, 2, 3)}
    rq = O.ref_feature_quarter({l: t["feats"][l].view(b, v, *feats[l].shape[1:])[:, 0] for l in (1, 2, 3)})   # (no graph: a leaf below)
    ref_q = torch.cat([rq[1], rq[2], rq[3]], 1).permute(0, 2, 3, 1).contiguous().requires_grad_(True)   # [B,h,w,96]
    assert ref_q.is_leaf
    h, w = ref_q.shape[1:3]
    nd, vw = t["iters"][it]["nd_in"], t["view_w"]
    samples = O.iteration_depth_samples(nd, inv_min.view(b, 1, 1, 1), inv_max.view(b, 1, 1, 1))
    off, chans, loss = {1: 0, 2: 16, 3: 48}, {1: 16, 2: 32, 3: 48}, 0
    for i, l in enumerate((1, 2, 3)):
        refl = ref_q[..., off[l]:off[l] + chans[l]].permute(0, 3, 1, 2)
        acc, wsum = 0, 1e-5
        for s, corr in enumerate(_oracle_corr_views(pv[l], refl, p12[i], samples[l], feats[l].shape[2:])):
            wv = vw[:, s].view(b, 1, 1, h, w)
            acc, wsum = acc + corr * wv, wsum + wv
        agg = acc / wsum
        want_agg = t["iters"][it]["aggs"][i]
        assert float((agg.detach() - want_agg).abs().max()) <= 1e-5 * max(1.0, float(want_agg.abs().max()))   # the traced call, restated
        loss = loss + (agg * t["iters"][it]["up"][i]).sum()
    loss.backward()
    dev = lambda x: x.to("cuda")
    fg = {l: dev(t["feats"][l]).contiguous(memory_format=torch.channels_last).requires_grad_(True) for l in (1, 2, 3)}
    stored = None if storage == "fp32" else {l: fg[l].detach().to(STORAGE[storage]) for l in fg}
    if stored is not None:
        assert all(torch.equal(stored[l].float(), fg[l].detach()) for l in fg)                   # the oracle's storage model == 16-bit values
    rqd = dev(ref_q.detach()).requires_grad_(True)
    outs = ops.corr_iter_train(fg, b, v, rqd, dev(p12), dev(vw), dev(inv_min), dev(inv_max), dev(nd), sample_offsets(), stored=stored)
    worst = 0.0
    for o, i in zip(outs, range(3)):
        want = t["iters"][it]["aggs"][i].permute(0, 2, 1, 3, 4)
        worst = max(worst, float((o.detach().cpu() - want).abs().max()) / max(1.0, float(want.abs().max())))
    assert worst <= 5e-5, worst                                                                  # forward, like the inference gate
    sum((o * dev(t["iters"][it]["up"][i].permute(0, 2, 1, 3, 4))).sum() for i, o in enumerate(outs)).backward()
    rep = {}
    for l in (1, 2, 3):
        g_ref = feats[l].grad
        scale = max(1e-30, float(g_ref.abs().max()))
        rep[l] = float((fg[l].grad.cpu() - g_ref).abs().max()) / scale
        assert rep[l] <= 1e-4, (l, rep[l], scale)
        assert float(fg[l].grad.reshape(b, v, -1)[:, 0].abs().max()) == 0.0                     # reference view: through ref_q only
    scale = max(1e-30, float(ref_q.grad.abs().max()))
    rep["ref_q"] = float((rqd.grad.cpu() - ref_q.grad).abs().max()) / scale
    assert rep["ref_q"] <= 1e-4, rep
    print(f"teacher-forced backward, iteration {it}, {storage}: forward {worst:.1e}, gradients (max abs / scale) {rep}")


@pytest.mark.parametrize("storage", ["fp32", "bf16", "fp16"])
def test_corr_init_backward_on_the_oracles_training_features(cfg4_backward_trace, storage):
    """itermvs_corr_init_backward at the cfg-4 size (level 3: 64x80, 32 planes, B = 2, 4 source views) on the oracle's
    FeatureNet output; upstream gradient: seeded noise (the per-view volumes are not a traced seam of the oracle)"""
    from itermvs_amd import ops
    traces, p12, inv_min, inv_max = cfg4_backward_trace
    b, v = 2, 5
    f3 = traces[storage]["feats"][3].clone().requires_grad_(True)
    h3, w3 = f3.shape[2:]
    depth = O.initial_depth_samples(inv_min.view(b, 1, 1, 1), inv_max.view(b, 1, 1, 1), h3, w3)
    gw = torch.randn((b, v - 1, 32, 8, h3, w3), generator=torch.Generator().manual_seed(5))
    pv = f3.view(b, v, *f3.shape[1:])
    corrs = _oracle_corr_views(pv, pv[:, 0], p12[2], depth, (h3, w3))
    sum((c.permute(0, 2, 1, 3, 4) * gw[:, s]).sum() for s, c in enumerate(corrs)).backward()
    fg = f3.detach().to("cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
    stored = None if storage == "fp32" else fg.detach().to(STORAGE[storage])
    assert stored is None or torch.equal(stored.float(), fg.detach())
    out = ops.corr_init_train(fg, b, v, p12[2].to("cuda"), inv_min.to("cuda"), inv_max.to("cuda"), 32, stored=stored)
    want = torch.stack([c.detach().permute(0, 2, 1, 3, 4) for c in corrs], 1)
    assert float((out.detach().cpu() - want).abs().max()) <= 5e-5 * max(1.0, float(want.abs().max()))
    (out * gw.to("cuda")).sum().backward()
    scale = float(f3.grad.abs().max())
    err = float((fg.grad.cpu() - f3.grad).abs().max()) / scale
    assert err <= 1e-4, (err, scale)
    print(f"teacher-forced init backward, {storage}: {err:.1e} of the gradient scale {scale:.3g}")
