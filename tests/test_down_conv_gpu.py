"""itermvs_down_conv (csrc/down_conv.hip): the stride-2 pair of a FeatureNet residual block -- conv1 + ReLU and the
down-sampling shortcut -- in one cooperative launch, against torch in fp64 and against the itermvs_conv2d launch it replaces."""
import pytest
import torch
import torch.nn.functional as F

import walk_shapes

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRS = [(16, 32), (32, 48)]        # (Cin, C): layer2.0 and layer3.0
TILE_ROWS, TILE_COLS = {16: 4, 32: 2}, 16        # output pixels of a tile in down_conv.hip (itermvs_down_conv: TH by Cin)


def ops():
    from itermvs_amd import ops as _ops
    return _ops


def rel_err(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-6))


def make(cin, c, n, h, w, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + cin * 1000 + n * 100 + h)
    x = torch.randn((n, cin, h, w), generator=g).relu().to(DEV)
    wt = (torch.randn((2 * c, cin, 3, 3), generator=g) / (cin * 9) ** 0.5).to(DEV)
    b = (torch.randn((2 * c,), generator=g) * 0.2).to(DEV)
    return x, wt, b


def reference(x, wt, b, c):
    """fp64: y = relu(conv(x; W1) + b1), sc = conv(x; Wd) + bd"""
    r = F.conv2d(x.double(), wt.double(), None if b is None else b.double(), stride=2, padding=1)
    return F.relu(r[:, :c]), r[:, c:]


def persistent_shape(cin):
    """Smallest (3, H, 34) whose tile list is longer than the launcher's persistent grid AND gives one workgroup a run of tiles
    that crosses an image boundary.  Mirrors launch_down: tiles = N * ceil(Ho / TH) * ceil(Wo / 16), grid = min(tiles, CUs)
    rounded down to a multiple of 8, workgroup g owns tiles [g * run + min(g, extra), ...) with run = tiles // grid and the
    first extra = tiles % grid workgroups one more.  W = 34 makes two tile columns, the second one a single pixel wide."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, w = 3, 34
    for h in range(2, 4096, 2):
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        per = -(-ho // TILE_ROWS[cin]) * -(-wo // TILE_COLS)
        tiles = n * per
        grid = min(tiles, cus)
        if grid >= 16:
            grid &= ~7
        if tiles <= grid:
            continue
        run, extra = divmod(tiles, grid)
        for g in range(grid):
            t0 = g * run + min(g, extra)
            t1 = t0 + run + (1 if g < extra else 0)
            if any(t0 < k * per < t1 for k in range(1, n)):
                return n, h, w
    raise AssertionError("no shape found")


SHAPES = [(1, 2, 2),        # smaller than any tile, every tap but the centre padded
          (1, 9, 33),       # odd sizes, one pixel past a 16-wide segment
          (2, 38, 70),      # ragged in both directions, several tiles, two images
          (3, 64, 96),      # whole tiles, more than one tile per column
          "persistent"]     # more tiles than workgroups: a workgroup walks several tiles and crosses an image boundary
SHAPES += list(walk_shapes.REGIMES)     # the regimes of the tile walk (TILE_ROWS x 16 output pixels per tile)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_down_conv_matches_fp64_and_the_conv2d_launch(pair, shape):
    """both results within 3e-6 of torch's fp64 convolution and within 2e-6 of this library's fp32-MFMA launch"""
    cin, c = pair
    if shape in walk_shapes.REGIMES:
        n, ho, wo = walk_shapes.walk_shape(shape, TILE_ROWS[cin], TILE_COLS)
        shape = (n, 2 * ho, 2 * wo - 1)
    n, h, w = persistent_shape(cin) if shape == "persistent" else shape
    x, wt, b = make(cin, c, n, h, w)
    want_y, want_s = reference(x, wt, b, c)
    y, sc = ops().down_conv(x, ops().MfmaWeight(wt, split3=True), b, c)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert y.shape == sc.shape == (n, c, ho, wo)
    ey, es = rel_err(y, want_y), rel_err(sc, want_s)
    old_s = torch.empty_like(sc)
    old_y = ops().conv2d(x, ops().MfmaWeight(wt, split3=False), b, stride=2, act="relu", split=(c, "none", old_s))
    oy, os_ = rel_err(y, old_y), rel_err(sc, old_s)
    print(f"down_conv {pair} {(n, h, w)}: vs fp64 y {ey:.2e} sc {es:.2e}; vs conv2d y {oy:.2e} sc {os_:.2e}")
    assert ey <= 3e-6 and es <= 3e-6, (ey, es)
    assert oy <= 2e-6 and os_ <= 2e-6, (oy, os_)


@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_down_conv_strides_and_neighbours(pair):
    """input and both outputs as channel slices of larger buffers: bit for bit the dense call, nothing written outside"""
    cin, c = pair
    n, h, w = 2, 38, 70
    x, wt, b = make(cin, c, n, h, w, seed=1)
    pk = ops().MfmaWeight(wt, split3=True)
    y, sc = ops().down_conv(x, pk, b, c)
    big_x = torch.zeros((n, cin + 4, h, w), device=DEV)
    big_x[:, 2:2 + cin] = x
    big_y = torch.zeros((n, c + 3, y.shape[2], y.shape[3]), device=DEV)
    big_s = torch.zeros((n, c + 5, y.shape[2], y.shape[3]), device=DEV)
    y2, s2 = ops().down_conv(big_x[:, 2:2 + cin], pk, b, c, out=big_y[:, 1:1 + c], out_b=big_s[:, 3:3 + c])
    assert torch.equal(y2, y) and torch.equal(s2, sc)
    assert torch.equal(big_y[:, 1:1 + c], y) and torch.equal(big_s[:, 3:3 + c], sc)
    assert float(big_y[:, :1].abs().max()) == 0.0 and float(big_y[:, 1 + c:].abs().max()) == 0.0
    assert float(big_s[:, :3].abs().max()) == 0.0 and float(big_s[:, 3 + c:].abs().max()) == 0.0


@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_down_conv_padding_is_zero(pair):
    """ones times ones: every output is (number of in-image taps) * Cin exactly -- 4 in the corners, 6 on the edges, 9 inside"""
    cin, c = pair
    n, h, w = 1, 9, 37
    x = torch.ones((n, cin, h, w), device=DEV)
    wt = torch.ones((2 * c, cin, 3, 3), device=DEV)
    y, sc = ops().down_conv(x, ops().MfmaWeight(wt, split3=True), None, c)
    rows = torch.tensor([sum(0 <= 2 * o - 1 + k < h for k in range(3)) for o in range(y.shape[2])], device=DEV)
    cols = torch.tensor([sum(0 <= 2 * o - 1 + k < w for k in range(3)) for o in range(y.shape[3])], device=DEV)
    want = (rows[:, None] * cols[None, :] * cin).float().expand_as(y)
    assert torch.equal(y, want) and torch.equal(sc, want)
    assert float(y[0, 0, 0, 0]) == 4 * cin and float(y[0, 0, -1, -1]) == 4 * cin      # odd sizes: all four corners see 2 x 2 taps
    assert float(y[0, 0, 0, 1]) == 6 * cin and float(y[0, 0, 1, 0]) == 6 * cin and float(y[0, 0, 1, 1]) == 9 * cin


@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_down_conv_extremes_survive_the_split(pair):
    """one image scaled by 3e4, one by 1e-30: the three-term split is exact, so each image keeps the fp64 bound on its own"""
    cin, c = pair
    n, h, w = 2, 38, 70
    x, wt, _ = make(cin, c, n, h, w, seed=2)
    x = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    x[0] *= 3e4
    x[1] *= 1e-30
    want_y, want_s = reference(x, wt, None, c)
    y, sc = ops().down_conv(x, ops().MfmaWeight(wt, split3=True), None, c)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(sc).all())
    for i in range(n):
        rel = lambda a, r: float((a[i].double() - r[i]).abs().max() / r[i].abs().max())
        ey, es = rel(y, want_y), rel(sc, want_s)
        print(f"down_conv {pair} extremes image {i}: y {ey:.2e} sc {es:.2e}")
        assert ey <= 3e-6 and es <= 3e-6, (i, ey, es)


def test_down_conv_errors():
    x, wt, b = make(24, 32, 1, 8, 8)
    with pytest.raises(RuntimeError):
        ops().down_conv(x, ops().MfmaWeight(wt, split3=True), b, 32)
    x, wt, b = make(16, 32, 1, 8, 8)
    with pytest.raises(RuntimeError):
        ops().down_conv(x, ops().MfmaWeight(wt, split3=False), b, 32)


def test_down_conv_in_the_engine(monkeypatch):
    """feature_net with the stride-2 blocks through down_conv against the same engine with them through the itermvs_conv2d
    launch: all three pyramid levels within 5e-6 (the single-layer figure with room for the layers behind it)"""
    from itermvs_amd import synthetic
    from itermvs_amd.engine import InferenceEngine
    from itermvs_amd.net import Pipeline
    model = Pipeline(iteration=2, test=True)
    model.load_state_dict(synthetic.random_state_dict(0))
    model = model.to(DEV).eval()
    x = torch.rand((2, 3, 64, 96), generator=torch.Generator().manual_seed(3)).to(DEV)
    calls = []
    real = ops().down_conv

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    def old_launch(x, packed, bias, c, out=None, out_b=None):
        return ops().conv2d(x, packed, bias, stride=2, act="relu", out=out, split=(c, "none", out_b)), out_b

    with torch.no_grad():
        monkeypatch.setattr(ops(), "down_conv", counted)
        new = {l: f.float().clone() for l, f in InferenceEngine(model.weights(), 2, conv_arithmetic="bf16x3").feature_net(x).items()}
        assert len(calls) == 2          # layer2.0 and layer3.0
        monkeypatch.setattr(ops(), "down_conv", old_launch)
        old = {l: f.float().clone() for l, f in InferenceEngine(model.weights(), 2, conv_arithmetic="bf16x3").feature_net(x).items()}
    for l in (1, 2, 3):
        e = rel_err(new[l], old[l])
        print(f"feature_net level {l}: down_conv vs conv2d launch {e:.2e}")
        assert e <= 5e-6, (l, e)
