"""The memory-less segments of a mixed call without a GPU: the planner (csrc/walk_plan.h: plan_dfa_items, run by
tests/emul/dfa_plan_emul.cpp) and the host build of the multi-table kernel's per-item walk (csrc/dfa_mixed_core.h, run one lane at a
time by tests/emul/dfa_mixed_emul.cpp) against the golden answers.  The kernel around them is checked by tests/test_mixed_dfa_gpu.py."""
import json
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import image
from testlib import MANIFEST, MAX_BYTES, emul_exe, fixture_blob

SLICE, MAX_ITEMS, OWN_DEFAULT = 256, 96, 32768      # walk_plan.h: kDfaSliceStrings, kDfaMaxItems, kDfaOwnDefault
ROW, TILE = 258, 4 * 64 * 144                       # dfa_split_core.h: kDfaRow; dfa_mixed_core.h: kMixTileBytes
NFA = [a for a in MANIFEST["automata"] if a["name"].startswith("nfa_")]


@pytest.fixture(scope="module")
def plan_emul():
    return emul_exe("dfa_plan")


@pytest.fixture(scope="module")
def walk_emul():
    return emul_exe("dfa_mixed")


def table_bytes(states):
    return states * ROW * 2


def img(kind, states=6, rev=0):
    """kind: "mem" a memory automaton; "dfa" a memory-less one -- eligible by the rule of launch_dfa_walk: 16-bit pre-multiplied states
    and table plus tile within 64 KiB"""
    if kind == "mem":
        return (0, 0, 0, 0)
    eligible = states * ROW <= 0xffff and table_bytes(states) + TILE <= 64 * 1024
    return (1, int(eligible), rev, table_bytes(states))


def run_plan(exe, seg_first, imgs, table_schedule=1, env=("MFA_MIXED_DFA=1",)):
    """env: the knobs; the multi-table launch is asked for unless a case says otherwise (it is off by default: test_knobs_move_segments)"""
    line = "%s %s %d %s\n" % (",".join(str(x) for x in seg_first), ";".join(",".join(str(v) for v in i) for i in imgs), table_schedule, " ".join(env))
    p = subprocess.run([exe], input=line.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    return json.loads(p.stdout)


def check_cover(plan, seg_first, imgs):
    """every string of every memory-less segment in exactly one item or one own-launch segment; no item crosses a segment, touches a
    memory segment, holds an ineligible image or is empty; the items' table fits beside the tile"""
    n = seg_first[-1]
    seen = np.zeros(n, dtype=np.int32)
    for image_k, first, count in plan["items"]:
        assert count > 0 and seg_first[image_k] <= first and first + count <= seg_first[image_k + 1], "an item crosses its segment"
        assert imgs[image_k][0] == 1 and imgs[image_k][1] == 1, "a memory automaton or an ineligible image in an item"
        assert imgs[image_k][3] <= plan["table_bytes"] and plan["table_bytes"] + TILE <= 64 * 1024
        seen[first:first + count] += 1
    assert len(set(plan["own"])) == len(plan["own"])
    for s in plan["own"]:
        assert imgs[s][0] == 1 and seg_first[s + 1] > seg_first[s]
        seen[seg_first[s]:seg_first[s + 1]] += 1
    want = np.zeros(n, dtype=np.int32)
    for s, i in enumerate(imgs):
        if i[0] == 1:
            want[seg_first[s]:seg_first[s + 1]] = 1
    assert np.array_equal(seen, want)
    assert plan["strings"] == sum(c for _, _, c in plan["items"]) and plan["slices"] == sum((c + SLICE - 1) // SLICE for _, _, c in plan["items"])
    assert plan["launches"] == (len(plan["items"]) + MAX_ITEMS - 1) // MAX_ITEMS
    # the workgroups' runs of slices tile [0, slices) in order
    assert plan["wg"][0] == 0 and plan["wg"][-1] == plan["slices"] and all(a <= b for a, b in zip(plan["wg"], plan["wg"][1:]))


def test_plan_covers_every_memoryless_string_once(plan_emul):
    rng = np.random.default_rng(5)
    for _ in range(60):
        ns = int(rng.integers(1, 40))
        imgs = [img(str(rng.choice(["mem", "dfa"])), int(rng.choice([2, 6, 30, 55, 56, 127, 128, 254, 255, 5000])), int(rng.integers(0, 2))) for _ in range(ns)]
        counts = [int(rng.choice([0, 0, 1, 7, 255, 256, 257, 4096, 40000])) for _ in range(ns)]
        seg_first = [0] + [int(x) for x in np.cumsum(counts)]
        plan = run_plan(plan_emul, seg_first, imgs)
        check_cover(plan, seg_first, imgs)
        assert plan["multi"] == 1 and plan["own_min"] == OWN_DEFAULT
        for s in range(ns):
            if imgs[s][0] == 1 and counts[s]:
                assert (s in plan["own"]) == (not imgs[s][1] or counts[s] >= OWN_DEFAULT), (s, imgs[s], counts[s])


def test_empty_segments_and_memory_segments_yield_nothing(plan_emul):
    imgs = [img("dfa"), img("mem"), img("dfa", 9, 1), img("dfa"), img("mem"), img("dfa")]
    seg_first = [0, 0, 500, 800, 800, 900, 900]                      # empty at the start, in the middle and at the end
    plan = run_plan(plan_emul, seg_first, imgs)
    assert plan["items"] == [[2, 500, 300]] and plan["own"] == [] and plan["table_bytes"] == table_bytes(9)
    check_cover(plan, seg_first, imgs)
    plan = run_plan(plan_emul, [0, 10, 20], [img("mem"), img("mem")])
    assert plan["items"] == [] and plan["own"] == [] and plan["slices"] == 0


def test_knobs_move_segments(plan_emul):
    imgs = [img("dfa", 5), img("mem"), img("dfa", 7, 1), img("dfa", 200), img("dfa", 40000)]
    seg_first = [0, 100, 200, 1200, 1300, 1400]
    plan = run_plan(plan_emul, seg_first, imgs)
    assert [i[0] for i in plan["items"]] == [0, 2] and plan["own"] == [3, 4]       # beyond 64 KiB with the tile; table in L2
    check_cover(plan, seg_first, imgs)
    for env in (["MFA_MIXED_DFA=0"], []):                                           # off, and the default: off as well
        off = run_plan(plan_emul, seg_first, imgs, env=env)
        assert off["items"] == [] and off["own"] == [0, 2, 3, 4] and off["multi"] == 0
        check_cover(off, seg_first, imgs)
    own = run_plan(plan_emul, seg_first, imgs, env=["MFA_MIXED_DFA=1", "MFA_MIXED_DFA_OWN=1000"])      # the segment of 1000 strings moves, the one of 100 stays
    assert [i[0] for i in own["items"]] == [0] and own["own"] == [2, 3, 4] and own["own_min"] == 1000
    own = run_plan(plan_emul, seg_first, imgs, env=["MFA_MIXED_DFA=1", "MFA_MIXED_DFA_OWN=1001"])
    assert [i[0] for i in own["items"]] == [0, 2] and own["own"] == [3, 4]
    # the per-segment schedule (MFA_WALK=jit): every memory-less segment in a launch of its own
    jit = run_plan(plan_emul, seg_first, imgs, table_schedule=0)
    assert jit["items"] == [] and jit["own"] == [0, 2, 3, 4]
    check_cover(jit, seg_first, imgs)


def test_an_item_has_one_direction_and_one_image(plan_emul):
    imgs = [img("dfa", 4, k % 2) for k in range(30)]
    seg_first = [300 * k for k in range(31)]
    plan = run_plan(plan_emul, seg_first, imgs)
    check_cover(plan, seg_first, imgs)
    # an item is one segment's: its direction is its image's, forward and reversed neighbours never share one
    assert [i[0] for i in plan["items"]] == list(range(30))
    for image_k, first, count in plan["items"]:
        assert first == seg_first[image_k] and count == 300


def test_more_items_than_a_launch_takes(plan_emul):
    imgs = [img("dfa", 3) for _ in range(2 * MAX_ITEMS + 5)]
    seg_first = list(range(len(imgs) + 1))
    plan = run_plan(plan_emul, seg_first, imgs)
    check_cover(plan, seg_first, imgs)
    assert len(plan["items"]) == len(imgs) and plan["launches"] == 3


def other_direction(name):
    """the fixture's image made to scan in the other direction than its own (it then accepts the mirrored strings)"""
    return fixture_blob(name, 1 - image.blob_info(fixture_blob(name))["reversed"])


def test_item_walk_on_every_fixture(walk_emul, tmp_path):
    """all 26 nfa_* fixtures, in their own scan direction and in the other one (then on the mirrored strings: the same answers), over their
    abc7 / rnd / odd sets as ONE item list in one batch; between the segments lie strings no item holds"""
    assert len(NFA) == 26
    strings, items, want, blobs = [], [], [], []
    gap = [b"never walked", b"", b"x" * 300]
    for rev in (0, 1):
        for a in NFA:
            assert sorted(a["sets"]) == ["abc7", "odd", "rnd"]
            (tmp_path / ("%d.blob" % len(blobs))).write_bytes(other_direction(a["name"]) if rev else fixture_blob(a["name"]))
            first = len(strings)
            for sset in ("abc7", "odd", "rnd"):
                ss = oracle_lib.load_set(sset)
                strings += [s[::-1] for s in ss] if rev else ss
                want += [int(b) for b in oracle_lib.load_bits(a["name"], sset)]
            items.append((first, len(strings) - first, len(blobs)))
            blobs.append(str(tmp_path / ("%d.blob" % len(blobs))))
            strings += gap
            want += [-1] * len(gap)
    data, off = oracle_lib.pack(strings)
    assert {int(o) % 16 for o in off[:-1]} == set(range(16))
    (tmp_path / "batch.bin").write_bytes(struct.pack("<QQ", len(strings), len(items)) + off.astype("<u8").tobytes()
                                         + b"".join(struct.pack("<QQQ", *i) for i in items) + data.tobytes()[:int(off[-1])])
    p = subprocess.run([walk_emul, str(tmp_path / "batch.bin")] + blobs, capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    lines = p.stdout.decode().split("\n")
    head = lines[0].split()
    assert int(head[1]) == 52 and int(head[3]) == sum((c + SLICE - 1) // SLICE for _, c, _ in items)      # one table fill per automaton
    got = np.array([-1 if x == "-" else int(x) for x in lines[1:1 + len(strings)]])
    bad = np.nonzero(got != np.array(want))[0]
    assert bad.size == 0, "%d differences, first: string %d %r want %d got %d" % (bad.size, bad[0], strings[bad[0]][:40], want[bad[0]], got[bad[0]])


def test_item_walk_lines_and_limits(walk_emul, tmp_path):
    """strings that start and end at every residue mod 16 and mod 128, lengths around the line size, both directions, against the CPU
    restatement; a string of exactly MFA_MAX_STRING_BYTES is walked, one byte more is answered 2"""
    rng = np.random.default_rng(77)
    blobs = [fixture_blob("nfa_abb_thompson", 0), fixture_blob("nfa_abb_thompson", 1), fixture_blob("nfa_star4_plain", 0), fixture_blob("nfa_third_glushkov", 1)]
    paths = []
    for k, b in enumerate(blobs):
        (tmp_path / ("%d.blob" % k)).write_bytes(b)
        paths.append(str(tmp_path / ("%d.blob" % k)))
    strings, items = [], []
    for k in range(len(blobs)):
        first = len(strings)
        for ln in [0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1024, 1025] + [int(x) for x in rng.integers(0, 600, size=300)]:
            t = bytes(rng.choice(list(b"ab" if ln % 4 else b"abc"), size=ln).tolist())
            if ln % 3 == 0 and ln >= 3:
                t = t[:-3] + b"abb" if k != 1 else b"bba" + t[3:]
            strings.append(t)
        items.append((first, len(strings) - first, k))
    limit = MAX_BYTES
    first = len(strings)
    strings += [b"ab" * ((limit - 3) // 2) + b"abb", b"a" * (limit + 1), b"abb"]
    items.append((first, 3, 0))
    data, off = oracle_lib.pack(strings)
    assert {int(o) % 128 for o in off[:-1]} >= set(range(0, 128, 9)) and {int(o) % 16 for o in off[:-1]} == set(range(16))
    want = np.zeros(len(strings), dtype=np.int64)
    for (f, c, k) in items[:-1]:
        want[f:f + c] = oracle_lib.OracleImage(blobs[k]).match(strings[f:f + c])
    want[first:] = [1, 2, 1]
    (tmp_path / "batch.bin").write_bytes(struct.pack("<QQ", len(strings), len(items)) + off.astype("<u8").tobytes()
                                         + b"".join(struct.pack("<QQQ", *i) for i in items) + data.tobytes()[:int(off[-1])])
    p = subprocess.run([walk_emul, str(tmp_path / "batch.bin")] + paths, capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    got = np.array([int(x) for x in p.stdout.decode().split("\n")[1:1 + len(strings)]])
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%d differences, first: string %d (len %d) want %d got %d" % (bad.size, bad[0], len(strings[bad[0]]), want[bad[0]], got[bad[0]])
    assert 0 < (want[:first] == 1).sum() < first


def test_eligibility_is_the_tiled_kernels_rule(walk_emul):
    """dfa_mixed_eligible itself: launch_dfa_walk gives dfa_tiled_kernel the images with 16-bit pre-multiplied states whose table plus
    the 36 864-byte tile is at most 64 KiB (kernels.hip) -- up to 55 state sets"""
    for states in (1, 2, 54, 55, 56, 57, 127, 128, 254, 255, 65535, 1 << 20):
        p = subprocess.run([walk_emul, "--eligible", str(states)], capture_output=True)
        assert p.returncode == 0, p.stderr.decode()
        flag, tb = (int(x) for x in p.stdout.split())
        assert tb == table_bytes(states) % (1 << 32)
        assert flag == int(states * ROW <= 0xffff and states * ROW * 2 + 4 * 64 * (128 + 16) <= 64 * 1024), states
        assert flag == img("dfa", states)[1] and flag == int(states <= 55)
