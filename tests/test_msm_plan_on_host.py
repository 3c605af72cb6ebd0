"""CPU-only: the MSM launch planner (scroll-prover_amd/csrc/msm_plan.hpp: window search, the plan of one pass, batch splitting, pipelined chunks, host slice cuts), compiled
into the stand-alone tests/hostcheck/msm_plan_main.cpp under -fsanitize=address,undefined and run as a program of its own.  Every field the program prints for a case is
compared with the restatement of tests/msm_plan_common.py: both sides of every window boundary in [2^11, 2^21], the sorter's tile edges, the sizes at which the coarse bins,
the 24 576-entry tile, the 16 384-entry level-2 tile and the segmented fix-up switch on, batches, tables, both record sizes, forced windows, a small device, every refusal and
every reason to split."""
import os
import subprocess

import pytest

from tests import msm_plan_common as mp

HERE = os.path.dirname(os.path.abspath(__file__))

BOUNDARIES = mp.boundaries(1 << 11, 1 << 21)
LENGTHS = sorted({n for b in BOUNDARIES for n in (b - 1, b)} | {16383, 16384, 16385, 32769, 49153, 100003, 1 << 22, 1 << 24, 1 << 26})
PLAN_FIELDS = ("n", "M", "c", "W", "fb", "cb_bits", "regions", "entries", "buckets")
RUN_FIELDS = ("seg", "blocks", "tn", "seg_arg", "big_cap", "huge_cap", "t1", "t2", "tiles1", "l2_tiles_max", "chunk", "chunks_per_set", "tree_quad_max")


def words(text):
    return "-" if text is None else text.replace(" ", "_")


def plan_line(n, M=1, tab_c=None, rec=144, forced=None, **settings):
    """(the program's input line, the line it must print) for one plan_pass case"""
    ask = dict(op="plan", n=n, M=M, tab_c=tab_c or 0, rec=rec, **settings)
    if forced:
        ask.update(forced_c=forced[0], forced_shared=int(forced[1]))
    p = mp.plan(n, M, tab_c, rec, forced, **settings)
    want = dict(refusal=words(p["refusal"]), must_split=int(p["must_split"]), shared=int(p["shared"]), **{f: p[f] for f in PLAN_FIELDS})
    if not p["refusal"]:
        want.update(fixup_kind=words(p["fixup_kind"]), quad_sums=int(p["sums"] == "quad"), quad_final=int(p["quad_final"]), **{f: p[f] for f in RUN_FIELDS})
    return ask, want


def cases():
    out = []
    for n in LENGTHS:
        for M in (1, 3, 9, 64):
            for tab_c in (None, 16, 17):
                for rec in (144, 256):
                    if rec == 256 and tab_c:
                        continue                                                   # the G2 MSM has no window tables
                    out.append(plan_line(n, M, tab_c, rec))
        for extra in ({"force_c": 4}, {"force_c": 24}, {"cus": 8}, {"no_tables": 1}):
            out.append(plan_line(n, 1, 16, **extra))
            out.append(plan_line(n, 3, None, 256, **extra))
    # every refusal, in the order plan_pass checks them, and every reason to split (a refusal | more than 2^29 entries | more than 8 GiB of bucket records)
    out.append(plan_line((1 << 31) - 1, 1, force_c=4))                              # n * windows >= 2^32
    out.append(plan_line(1 << 10, 1024, force_c=24))                                # too many buckets
    out.append(plan_line(1 << 10, 1024, force_c=16))                                # coarse histogram
    out.append(plan_line(1 << 10, 1, force_c=24, MI355_SORT_FB=9))                  # fb raised to kb - 11 = 12 is fine ...
    out.append(plan_line(1 << 10, 1, forced=(25, True)))                            # ... a 25-bit window is out of the sorter's range
    out.append(plan_line(1 << 26, 2))                                               # entries
    out.append(plan_line(1 << 22, 9, force_c=22))                                   # bucket records (G1)
    out.append(plan_line(1 << 22, 5, rec=256, force_c=22))                          # bucket records (G2's are larger)
    # the knobs the plan reads, away from their defaults
    for extra in ({"MI355_FIXUP_MODE": 0}, {"MI355_FIXUP_MODE": 1}, {"MI355_SORT_SPLIT": 2}, {"MI355_SORT_T1": 8192}, {"MI355_SORT_T2": 16384}, {"MI355_TAIL_COOP_MASK": 0},
                  {"MI355_TAIL_COOP_MAX": 0}, {"MI355_SEG_FACTOR": 4, "MI355_SEG_FILL": 100, "MI355_SEG_MIN": 1}, {"MI355_REDUCE_MIN_CHUNK": 16, "MI355_REDUCE_CHAINS": 4096},
                  {"MI355_MSM_AUTO_MAX_C": 16}, {"MI355_FIXUP_SERIAL_MAX": 7, "MI355_FIXUP_LANES_MAX_LOG": 12}, {"MI355_SORT_FB": 9}):
        for n in (7709, 455420, 1 << 24, 1 << 26):
            out.append(plan_line(n, 1, **extra))
    out.append(plan_line(100003, 1, 16, forced=(mp.plan(455420)["c"], False)))      # a slice of a host-sliced MSM takes the biggest slice's shape
    out.append(plan_line(100003, 1, 16, forced=(16, True)))
    # the batch splitter: an n = 2^26 batch of 64 halves down
    for n, M, rec in ((1 << 26, 64, 144), (1 << 22, 64, 144), (1 << 22, 64, 256), (100003, 9, 144)):
        out.append((dict(op="leaves", n=n, M=M, rec=rec), dict(leaves=",".join(map(str, mp.batch_leaves(n, M, None, rec))))))
    # pipelined chunks at both sides of the threshold (and of the quarter-threshold rule)
    for chunks in (1, 2, 4, 16):
        for min_log in (15, 23):
            for n in ((1 << min_log) - 1, 1 << min_log, (1 << min_log) + 1, 3 << min_log, 4 << min_log):
                for M in (1, 2):
                    kw = dict(MI355_MSM_CHUNKS=chunks, chunk_min_log=min_log)
                    out.append((dict(op="chunks", n=n, M=M, **kw), dict(chunks=mp.pipeline_chunks(n, M, **kw))))
    # host slices
    for n, M, tab_c, kw in [((1 << 22) - 1, 1, None, {}), (1 << 22, 1, None, {}), ((1 << 22) + 1, 1, None, {}), (1 << 26, 1, None, {}), (1 << 26, 1, 17, {}), (1 << 26, 2, None, {}),
                            ((1 << 20) + 3, 1, None, {"MI355_HOST_SLICE_MIN_LOG": 20}), (100003, 1, None, {"MI355_HOST_SLICE_MIN_LOG": 14, "MI355_HOST_CHUNKS": 4}),
                            (1 << 26, 1, None, {"MI355_HOST_CHUNKS": 1}), (1 << 26, 1, None, {"MI355_HOST_CHUNKS": 2}), (1 << 26, 1, None, {"MI355_HOST_CHUNKS": 64}),
                            (1 << 26, 1, None, {"force_c": 24}), (17, 1, None, {"MI355_HOST_SLICE_MIN_LOG": 4})]:
        cut, shape = mp.host_slices(n, M, tab_c, **kw)
        want = dict(cuts=",".join(map(str, cut)), slices=len(cut) - 1, shape_c=shape["c"] if shape else 0, shape_shared=int(shape["shared"]) if shape else 0,
                    shape_buckets=shape["buckets"] if shape else 0)
        out.append((dict(op="slices", n=n, M=M, tab_c=tab_c or 0, **kw), want))
    # mi355_srs_precompute's automatic window and its rule for tables that exist
    for n in (1 << 17, 1 << 18, 1 << 12, 1 << 26):
        best = mp.table_c(n)
        for have in (0, 12, best - 1, best, best + 1, 22):
            out.append((dict(op="window", n=n, have_c=have), dict(best=best, keep=int(bool(have) and mp.tables_close_enough(n, have, best)))))
    return out


CASES = cases()


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msmplan") / "msm_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "hostcheck", "msm_plan_main.cpp")])
    text = "".join(" ".join("%s=%s" % kv for kv in ask.items()) + "\n" for ask, _ in CASES)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES)
    return [dict(w.split("=", 1) for w in line.split()) for line in lines]


def test_the_cases_reach_every_switch_of_the_planner():
    """what the case list is made for; the figures are today's defaults (the issue's list of boundaries)"""
    assert BOUNDARIES == [2402, 7709, 13639, 39138, 71160, 128087, 455420, 1707824]
    plans = [want for ask, want in CASES if ask["op"] == "plan"]
    assert {p["refusal"] for p in plans} == {"-"} | {words(t) for t in mp.REFUSALS.values()}
    ok = [p for p in plans if p["refusal"] == "-"]
    assert {p["fixup_kind"] for p in ok} == {"segmented", "quad", "four_lanes", "one_lane"}
    assert {p["t1"] for p in ok} == {8192, 16384, 24576} and {p["t2"] for p in ok} == {8192, 16384}
    assert {p["quad_sums"] for p in ok} == {0, 1} and {p["quad_final"] for p in ok} == {0, 1} and {min(p["cb_bits"], 1) for p in ok} == {0, 1}
    assert {p["shared"] for p in ok} == {0, 1} and {p["seg"] for p in ok} >= {16, 4096} and {p["chunk"] for p in ok} >= {4, 8, 16, 32}
    assert any(p["must_split"] and p["refusal"] == "-" for p in plans)
    first = mp.plan(1 << 22), mp.plan(1 << 24), mp.plan(1 << 26)
    assert [p["cb_bits"] > 0 for p in first] == [True] * 3 and [p["t1"] for p in first] == [24576] * 3 and [p["t2"] for p in first] == [8192, 16384, 16384]
    assert [p["fixup_kind"] == "segmented" for p in first] == [False, False, True]
    assert mp.batch_leaves(1 << 26, 64) == [1] * 64 and mp.batch_leaves(1 << 22, 64) == [8] * 8 and mp.table_c(1 << 17) == 16 and mp.table_c(1 << 18) == 17
    assert {want["chunks"] for ask, want in CASES if ask["op"] == "chunks"} >= {1, 2, 4, 12, 16}   # 12: sixteen chunks asked for, a quarter of the threshold each allows twelve
    assert {want["slices"] for ask, want in CASES if ask["op"] == "slices"} >= {1, 2, 4, 5}
    assert {want["keep"] for ask, want in CASES if ask["op"] == "window"} == {0, 1}


def test_host_slice_cuts_are_strictly_increasing_and_aligned():
    for ask, want in CASES:
        if ask["op"] != "slices":
            continue
        cut = [int(c) for c in want["cuts"].split(",")]
        assert cut[0] == 0 and cut[-1] == ask["n"] and all(a < b for a, b in zip(cut, cut[1:])), (ask, cut)
        if ask["n"] >= 1 << 20:
            assert all(c % 1024 == 0 for c in cut[1:-1]), (ask, cut)
    assert mp.host_slices(1 << 26, MI355_HOST_CHUNKS=1)[0] == [0, 1 << 26] and mp.host_slices((1 << 22) - 1)[0] == [0, (1 << 22) - 1]
    assert len(mp.host_slices(1 << 22)[0]) > 2 and len(mp.host_slices((1 << 20) + 3, MI355_HOST_SLICE_MIN_LOG=20)[0]) > 2


@pytest.mark.parametrize("op", ["plan", "leaves", "chunks", "slices", "window"])
def test_planner_matches_the_restatement(printed, op):
    seen = 0
    for (ask, want), got in zip(CASES, printed):
        if ask["op"] != op:
            continue
        seen += 1
        assert got == {k: str(v) for k, v in want.items()}, (ask, {k: (got.get(k), str(v)) for k, v in want.items() if got.get(k) != str(v)}, set(got) - set(want))
    assert seen
