"""The launch planner (csrc/walk_plan.h, csrc/walk.h: pure functions, no HIP), compiled for the host (tests/emul/plan_emul.cpp), against
the plans recorded in tests/golden/plans/ -- what the commit before the planner was split from the launch code decided for the same
cases, field for field and return codes included -- and the invariants of the layout of a wave's memory.  What the kernels do with a
plan is checked by the GPU tests."""
import json
import os
import subprocess

import pytest

import oracle_lib
from testlib import emul_exe

PLANS = os.path.join(oracle_lib.GOLDEN, "plans")
LAUNCH_KEYS = ["g", "s0", "s1", "ml", "Kc", "w0", "w1", "a", "b", "k", "sf", "stb"]      # a recorded launch of a mixed call: these values, in this order
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
