"""The launch planner (csrc/walk_plan.h, csrc/walk.h: pure functions, no HIP), compiled for the host (tests/emul/plan_emul.cpp), against
the plans recorded in tests/golden/plans/ -- what the commit before the planner was split from the launch code decided for the same
cases, field for field and return codes included -- and the invariants of the layout of a wave's memory and of a mixed call's schedule.
mixed_schedule.jsonl holds whole schedules of mixed calls (region launches, events, walk launches, streams, the memory-less segments,
the reported counts): what the commit before plan_mixed put on its streams, its enqueue code run over stand-ins for the HIP calls.
What the kernels do with a plan is checked by the GPU tests."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from testlib import emul_exe

PLANS = os.path.join(oracle_lib.GOLDEN, "plans")
LAUNCH_KEYS = ["g", "s0", "s1", "ml", "Kc", "w0", "w1", "a", "b", "k", "sf", "stb"]      # a recorded launch of a mixed call: these values, in this order
MAX_LAUNCHES = 24                # a mixed object's launch slots (walk_plan.h: MIX_MAX_LAUNCHES)
LDS_LIMIT = 160 * 1024           # bytes of LDS of a CU (MI355X): a fact of the device, not read from the code under test


@pytest.fixture(scope="module")
def emul():
    return emul_exe("plan")


def recorded(name):
    with open(os.path.join(PLANS, name + ".jsonl")) as f:
        return [json.loads(line) for line in f]


def plans_of(emul, cases):
    p = subprocess.run([emul], input="\n".join(cases) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-400:]
    got = [json.loads(line) for line in p.stdout.splitlines()]
    assert len(got) == len(cases)
    return got


def test_walk_plans_equal_the_recorded_ones(emul):
    rec = recorded("walk")
    got = plans_of(emul, [r["case"] for r in rec])
    for r, g in zip(rec, got):
        g = {k: v for k, v in g.items() if k not in ("layout", "lean_layout")}
        assert g == r["plan"], r["case"]
    # the fixture does its job: every error the planner can return occurs, and so do all three kernels
    assert {r["plan"]["rc"] for r in rec} == {0, -1, -3, -6}
    assert {r["plan"].get("kernel", "")[:4] for r in rec} >= {"k1", "k9", "long", "stat"}


def test_mixed_plans_equal_the_recorded_ones(emul):
    rec = recorded("mixed")
    got = plans_of(emul, [r["case"] for r in rec])
    direct = 0
    for r, g in zip(rec, got):
        # one automaton in one group goes straight to the single-automaton call: the library plans no more than the cuts then, and
        # a call that has more launches than slots stops before streams are assigned
        keys = r["plan"].keys()
        g["launches"] = [[L[k] for k in LAUNCH_KEYS] for L in g["launches"]]
        direct += "launches" not in keys
        assert {k: g[k] for k in keys} == r["plan"], r["case"]
    assert 0 < direct < len(rec) // 4 and {len(r["plan"]["cut"]) - 1 for r in rec} >= {1, 5, 8, 12}
    assert {r["plan"]["rc"] for r in rec} == {0, -3}
    assert max(len(set(r["plan"].get("where", []))) for r in rec) == 4 and max(len(r["plan"].get("launches", [])) for r in rec) >= 20


def test_mixed_schedules_equal_the_recorded_ones(emul):
    rec = recorded("mixed_schedule")
    got = plans_of(emul, [r["case"] for r in rec])
    for r, g in zip(rec, got):
        # a call that is refused, or goes straight to the single-automaton call, was recorded as far as it got
        assert {k: g[k] for k in r["plan"]} == r["plan"], r["case"]
    # the fixture does its job: both engines, calibrated or not, the shortcut, a refusal, groups without a region launch, two region
    # launches in a group, objects without a memory automaton, multi-table launches in more than one piece, a shared stream
    plans = [r["plan"] for r in rec]
    assert {(p["table"], bool(any(p.get("where", [])))) for p in plans} == {(1, False), (0, False), (0, True)}
    assert {p["rc"] for p in plans} == {0, -3} and 3 <= sum(p.get("direct", 0) for p in plans) < len(plans) // 4
    whole = [p for p in plans if "regions" in p]
    assert len(whole) > 60 and any(p["NW"] == 0 and not p["regions"] for p in whole) and any(len(p["dfa_chunks"]) > 1 for p in whole)
    assert any(p["table"] and p["regions"] and 1 in p["own_event"] for p in whole) and any(p["KD"] == p["NW"] - 1 for p in whole if p["KD"] >= 0)
    assert any(sum(1 for r in p["regions"] if r[0] == 0) == 2 for p in whole) and any(p["NW"] and not p["regions"] for p in whole)


def images_of_case(case):
    """(memoryless?, first string, end) per segment of a `mixed` case line; whether the call scans regions"""
    f = case.split()
    flags = [(t.split(",") + ["0"] * 4)[4] == "1" for t in f[1].split(";")]
    seg_first = [int(x) for x in f[2].split(",")]
    scans = not ({"MFA_REGIONS=0", "MFA_ACCEL=0"} & set(f[9:])) and not all(flags)
    return [(m, a, b) for m, a, b in zip(flags, seg_first, seg_first[1:])], scans


def test_mixed_schedule_invariants(emul):
    """on every recorded case, old and new, from the planner's output alone"""
    cases = [r["case"] for r in recorded("mixed") + recorded("mixed_schedule")]
    checked = 0
    for case, g in zip(cases, plans_of(emul, cases)):
        counts = g["counts"]
        segs, scans = images_of_case(case)
        n = segs[-1][2]
        if g["rc"] != 0 or g["direct"]:
            assert not g["regions"] and not g["seg_walks"] and not g["dfa_items"] and not g["dfa_own"], case
            assert g["rc"] != 0 or (len(segs) == 1 and len(g["cut"]) == 2 and counts["groups"] == 1), case
            continue
        checked += 1
        cut = g["cut"]
        walks = [(L["g"], L["a"], L["b"], L["k"], L["waits"]) for L in g["launches"]] if g["table"] else [tuple(w[:1] + w[2:]) for w in g["seg_walks"]]
        memory = np.zeros(n, dtype=np.int32)
        for m, a, b in segs:
            memory[a:b] = 0 if m else 1
        # the region launches cover every string of a memory automaton exactly once and no other; none crosses its group; they are in order
        scanned, scanned_by = np.zeros(n, dtype=np.int32), np.full(n, len(cut), dtype=np.int32)
        for gr, a, b, threads, signals in g["regions"]:
            assert cut[gr] <= a < b <= cut[gr + 1] and threads == (128 if g["table"] else 256), case
            scanned[a:b] += 1
            scanned_by[a:b] = gr
        assert np.array_equal(scanned, memory if scans else 0 * memory), case
        assert [r[0] for r in g["regions"]] == sorted(r[0] for r in g["regions"]), case
        # a group's event: its last region launch's completion signal, or a record of its own -- one of the two, and only the last launch's
        for gr in range(len(cut) - 1):
            mine = [r for r in g["regions"] if r[0] == gr]
            assert [r[4] for r in mine[:-1]] == [0] * len(mine[:-1]) and (mine[-1][4] if mine else 0) + g["own_event"][gr] == 1, case
        # the walks cover every string of a memory automaton once, inside their group, and only strings whose regions a group no later
        # than their own has scanned; a stream's first walk of a group, and only that one, waits for the group's event
        walked, first = np.zeros(n, dtype=np.int32), set()
        for gr, a, b, k, waits in walks:
            assert cut[gr] <= a < b <= cut[gr + 1] and 0 <= k < g["NW"], case
            walked[a:b] += 1
            assert not scans or int(scanned_by[a:b].max()) <= gr, case
            assert waits == ((gr, k) not in first), case
            first.add((gr, k))
        assert np.array_equal(walked, memory), case
        assert [w[0] for w in walks] == sorted(w[0] for w in walks), case
        if g["table"]:
            assert [L["slot"] for L in g["launches"]] == list(range(len(walks))) and len(walks) <= MAX_LAUNCHES, case
        # the memory-less segments: a stream of their own while there is one, every item in exactly one multi-table launch
        has_dfa = bool(g["dfa_items"] or g["dfa_own"])
        assert g["KD"] == (min(g["NW"], 3) if has_dfa else -1) and g["NS"] == max(g["NW"], g["KD"] + 1) <= 4, case
        assert [c for ch in g["dfa_chunks"] for c in range(*ch)] == list(range(len(g["dfa_items"]))) and all(0 < b - a <= 96 for a, b in g["dfa_chunks"]), case
        # the reported counts are the lengths of the lists
        assert counts == {"region_launches": len(g["regions"]), "walk_launches": len(walks), "groups": len(cut) - 1, "dfa_multi": len(g["dfa_chunks"]),
                          "dfa_own": len(g["dfa_own"]), "dfa_items": len(g["dfa_items"]), "dfa_strings": sum(i[2] for i in g["dfa_items"]),
                          "no_regions": int(not g["regions"] and any(m for m, _, _ in segs))}, case
    assert checked > 100


def check_block(pieces, total):
    """the pieces follow each other without a gap or an overlap and add up to the block"""
    at = 0
    for name, first, words in pieces:
        assert first == at, (name, pieces)
        at += words
    assert at == total, pieces


def test_layout_invariants(emul):
    rec = recorded("walk")
    got = plans_of(emul, [r["case"] for r in rec])
    checked = 0
    for r, g in zip(rec, got):
        if g["rc"] != 0:
            continue
        checked += 1
        for key, lds_bytes in (("layout", g["lds_bytes"]), ("lean_layout", g["lean_lds_bytes"] if g["lean_grid"] else None)):
            lay = g[key]
            check_block(lay["lds"], lay["lds_words"])
            check_block(lay["spill"], lay["spill_used"])
            assert lay["spill_used"] <= lay["spill_words"], r["case"]
            if lds_bytes is not None:
                assert lds_bytes == 4 * (g["shared_words"] + 4 * lay["lds_words"]) <= LDS_LIMIT, r["case"]
        # every wave of either grid has its block inside the buffer, and the queue of string numbers lies behind them
        waves = max(4 * g["grid"] * g["layout"]["spill_words"], 4 * g["lean_grid"] * g["lean_layout"]["spill_words"] if g["lean_grid"] else 0)
        assert 4 * waves <= (g["queue_at"] if g["lean_grid"] else g["reserve_bytes"]) <= g["reserve_bytes"], r["case"]
    assert checked > 100
