"""Time itermvs_down_conv against the itermvs_conv2d launch it replaces (fp32 MFMA, two results), at FeatureNet's two stride-2
shapes of cfg 1 (5 x 16 x 256 x 320 -> 32 + 32 and 5 x 32 x 128 x 160 -> 48 + 48), 10 launches per hipGraph replay:
    python tools/down_conv_bench.py [--lib <other libitermvs_hip.so>]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from itermvs_amd import _lib
if "--lib" in sys.argv:
    _i = sys.argv.index("--lib")
    _lib.LIB_PATH = os.path.abspath(sys.argv[_i + 1])
    del sys.argv[_i:_i + 2]
from itermvs_amd import ops

dev = torch.device("cuda:0")


def timeit(run, reps=10, rounds=8):
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        gr.capture_begin()
        for _ in range(reps):
            run()
        gr.capture_end()
        best = 1e9
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    return best


print(f"library {_lib.LIB_PATH}")
for n, cin, c, h, w in ((5, 16, 32, 256, 320), (5, 32, 48, 128, 160)):
    g = torch.Generator().manual_seed(cin)
    x = torch.randn((n, cin, h, w), generator=g).relu().to(dev)
    wt = (torch.randn((2 * c, cin, 3, 3), generator=g) / (cin * 9) ** 0.5).to(dev)
    b = (torch.randn((2 * c,), generator=g) * 0.2).to(dev)
    pk3, pk = ops.MfmaWeight(wt, split3=True), ops.MfmaWeight(wt, split3=False)
    y, sc = (torch.empty((n, c, h // 2, w // 2), device=dev) for _ in range(2))
    y0, sc0 = torch.empty_like(y), torch.empty_like(sc)
    t_new = timeit(lambda: ops.down_conv(x, pk3, b, c, out=y, out_b=sc))
    t_old = timeit(lambda: ops.conv2d(x, pk, b, stride=2, act="relu", out=y0, split=(c, "none", sc0)))
    err = max(float((y - y0).abs().max() / y0.abs().max()), float((sc - sc0).abs().max() / sc0.abs().max()))
    print(f"{cin} -> {c}+{c}, {n} x {h} x {w}: down_conv {t_new:.1f} us   conv2d launch (fp32 MFMA) {t_old:.1f} us   "
          f"max |new - old| / max |old| = {err:.1e}")
