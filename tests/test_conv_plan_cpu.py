"""itermvs_conv2d_plan against recorded plans (tests/golden/conv_plan_cases.json), field for field, without a GPU.

The expectations were recorded from the commit BEFORE the plan existed: in a copy of that commit the final launch functions
(launch_direct, the three launch sites of conv_mfma.hip, launch_tile, launch_deconv, launch_tile3, launch_tile3_pair) wrote
their template arguments, LDS bytes and tile counts down instead of querying occupancy and launching, and every case ran
through that copy's itermvs_conv2d.  A case is the scalar fields of itermvs_conv_params plus which optional pointers are set;
it expects a status and, for status 0, the 22 fields of itermvs_conv_plan.  558 cases, packed as integer rows (see unpack).

GROUPS (the "group" of a case; counts are asserted by test_table_covers_every_branch)
  engine     every itermvs_conv2d call of InferenceEngine, logged on the GPU: both conv_arithmetic modes, the cfg-1, cfg-3 and
             cfg-5 shapes of bench.py, batch 1 and 2
  ragged     the same layers at 37x53 and 8x8 inputs with N = 1 and N = 7
  tile       weight_format 2: S = 1 / 2 / 4 (Cin 3, 8, 16..80), every line of the measured table and the inputs the generic
             search still decides, stride 2, dilation 2, split_cout with even and odd block counts, dot (act 6) with one and
             two blocks, LDS fall-backs to a narrower block (64 -> 64 and 80 -> 96 at stride 2), not covered: 1x1, stride 3,
             stride 2 + dilation 2, Cin <= 4 at stride 2, Cin 8 at dilation 2
  tile3      weight_format 3: every line of the table, CPS 1 / 2, split, dot, LDS fall-backs to a smaller tile and a
             narrower block, not covered: Cin <= 4, 1x1, layers whose weights exceed the LDS at every block width
  pair       the tap-pair form with planar and with channels-last input, MB 1 and 2 (dot), not covered: stride 2, split
  deconv     each of the six instantiations (MB 1 / 2 x (S 2, S 4 one chunk, S 4 two chunks)), not covered: Cin 4, Cin 48,
             three channel blocks, stride 1, pad 0, act 2; transposed in another weight format
  mfma       each {MB, NB} of conv_mfma_kernel that an input can select (seven of the nine) at 1x1 and 3x3, split-K with MB 1 and 2, the lateral-up2 case and its near misses
             (this back end covers every shape: it has no "not covered" answer)
  direct     each CT (1, 4, 8, 16, 32) of conv_direct_kernel at 1x1 and 3x3 (no "not covered" answer either)
"""
import ctypes as C
import json
import os
from collections import Counter

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_cases.json")
with open(GOLDEN) as _f:
    TABLE = json.load(_f)
SCALARS, FLAGS, TAGS, PLAN_FIELDS = TABLE["scalars"], TABLE["flags"], TABLE["tags"], TABLE["plan_fields"]


def unpack(group, row):
    """a row of the table: the scalars, seg_end[3], pointer flags (bits), engine tags (bits), fallback, status, then the plan"""
    n = len(SCALARS)
    case = dict(zip(SCALARS, row), group=group, seg_end=row[n:n + 3], fallback=row[n + 5], status=row[n + 6], plan=row[n + 7:])
    case.update({f: row[n + 3] >> i & 1 for i, f in enumerate(FLAGS)})
    case["tags"] = [t for i, t in enumerate(TAGS) if row[n + 4] >> i & 1]
    return case


CASES = [unpack(g, r) for g, rows in TABLE["groups"].items() for r in rows]
_BUF = (C.c_float * 64)()
ADDR = (C.addressof(_BUF) + 15) // 16 * 16          # a 16-byte aligned host address: the plan never reads through it


def make_params(case):
    """itermvs_conv_params of a case {field: value}: scalars as given, required pointers set, optional ones by their flag"""
    from itermvs_amd import _lib
    p = _lib.ConvParams()
    for f in SCALARS:
        setattr(p, f, case[f])
    for i in range(3):
        p.seg_end[i] = case["seg_end"][i]
        p.weight[i] = ADDR if i < case["n_seg"] else None
        p.bias[i] = ADDR if case["has_bias"] and i < case["n_seg"] else None
    p.inp = p.out = ADDR
    for f in ("out2", "add", "aux1", "aux2", "out_b"):
        setattr(p, f, ADDR if case["has_" + f] else None)
    hw = case["Hin"] * case["Win"]
    p.in_sn, p.out_sn, p.add_sn, p.aux1_sn, p.aux2_sn, p.out_b_sn = case["Cin"] * hw, case["Cout"] * hw, 0, 0, 0, 0
    return p


def run_plan(case):
    from itermvs_amd import _lib
    plan = _lib.ConvPlan()
    status = _lib.load().itermvs_conv2d_plan(C.byref(make_params(case)), C.byref(plan))
    return status, [getattr(plan, f) for f in PLAN_FIELDS]


@pytest.mark.parametrize("group", sorted(TABLE["groups"]))
def test_plan_matches_the_recorded_launches(group):
    from itermvs_amd import _lib
    assert PLAN_FIELDS == [n for n, _ in _lib.ConvPlan._fields_]
    bad = []
    for case in CASES:
        if case["group"] != group:
            continue
        status, plan = run_plan(case)
        want = case["plan"] if case["status"] == 0 else None
        if status != case["status"] or (want is not None and plan != want):
            bad.append((case, status, plan))
    assert not bad, f"{len(bad)} of group {group} differ, first: {bad[0]}"


def test_table_covers_every_branch():
    cases = CASES
    ok = [c for c in cases if c["status"] == 0]
    P = lambda c: dict(zip(PLAN_FIELDS, c["plan"]))
    groups = Counter(c["group"] for c in cases)
    assert set(groups) == {"engine", "ragged", "tile", "tile3", "pair", "deconv", "mfma", "direct"} and len(cases) == TABLE["count"]
    # the engine's calls: both arithmetic modes, three shapes, two batch sizes
    tags = {t for c in cases if c["group"] == "engine" for t in c["tags"]}
    assert tags == {f"{s}/{a}/b{b}" for s in ("cfg1", "cfg3", "cfg5") for a in ("bf16x3", "fp32") for b in (1, 2)}
    rag = [c for c in cases if c["group"] == "ragged"]
    assert {(c["Hin"], c["Win"], c["N"]) for c in rag} == {(h, w, n) for h, w in ((37, 53), (8, 8)) for n in (1, 7)}
    by = lambda b: [P(c) for c in ok if c["plan"][0] == b]
    assert {p["CT"] for p in by(0)} == {1, 4, 8, 16, 32} and {p["KS"] for p in by(0)} == {1, 3}
    # ({3, 1} and {2, 1} are instantiated but no input selects them: {1, 2} comes first and never has fewer waves)
    assert {(p["MB"], p["NB"]) for p in by(1)} == {(3, 4), (2, 4), (3, 2), (2, 2), (1, 4), (1, 2), (1, 1)}
    assert {p["MB"] for p in by(2)} == {1, 2} and by(3)
    tile = by(4)
    assert {p["S"] for p in tile} == {1, 2, 4} and {p["CPS"] for p in tile} == {1, 2, 3} and {p["MB"] for p in tile} == {1, 2, 3}
    assert {(p["STRIDE"], p["DIL"]) for p in tile} == {(1, 1), (2, 1), (1, 2)} and {(p["TH"], p["TWT"]) for p in tile} == {(8, 2), (4, 2), (4, 1)}
    assert {(p["MB"], p["S"], p["NCH"]) for p in by(5)} == {(m, s, n) for m in (1, 2) for s, n in ((2, 1), (4, 1), (4, 2))}
    t3 = by(6)
    # (CPS 3 needs ITERMVS_TILE3_FORCE: the table sends three-chunk layers to tiles whose three stages exceed the LDS budget)
    assert {p["CPS"] for p in t3} == {1, 2} and {p["MB"] for p in t3} >= {1, 2}
    assert {(p["STRIDE"], p["DIL"]) for p in t3} == {(1, 1), (2, 1), (1, 2)} and {(p["TH"], p["TWT"]) for p in t3} == {(8, 2), (4, 2), (4, 1)}
    assert {(p["MB"], p["INCL"]) for p in by(7)} == {(1, 0), (2, 0), (1, 1), (2, 1)}
    for fmt in (2, 3):
        mine = [c for c in cases if c["weight_format"] == fmt and not c["transposed"]]
        assert {c["act"] for c in mine if c["status"] == 0} >= {1, 6}                                      # dot ...
        assert {(c["Cout"] + 15) // 16 for c in mine if c["act"] == 6 and c["status"] == 0} == {1, 2}      # ... with mt 1 and 2
        assert {(c["split_cout"] // 16) % 2 for c in mine if c["split_cout"] and c["status"] == 0} == {0, 1}
        assert any(c["status"] == -2 for c in mine)                                                        # not covered
    assert any(c["status"] == -2 for c in cases if c["transposed"])
    # LDS fall-backs: the plan is narrower / smaller than the table's first choice for the layer
    fb = [c for c in cases if c.get("fallback")]
    assert {c["weight_format"] for c in fb} == {2, 3} and all(c["status"] == 0 for c in fb)
