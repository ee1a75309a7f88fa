"""Memory-less automata inside mixed batches (mfa_match_mixed): the multi-table launch (csrc/dfa_mixed.hip), the launches of single
segments, the clipped region pass, the scheduling around them and the command line, against the golden answers, the per-image calls and
the CPU restatement."""
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi
from testlib import DIPLOMA, MANIFEST, MAX_BYTES, filled, fixture_blob, front_end_blob, match_on_gpu, mixed_match, seg_first_of, upload

pytestmark = pytest.mark.gpu

NFA = [a for a in MANIFEST["automata"] if a["name"].startswith("nfa_")]
MEM = [a for a in MANIFEST["automata"] if a["name"].endswith("_plain") and a["name"].startswith("ex")][:10]


@pytest.fixture(autouse=True)
def multi_table_launch(monkeypatch):
    """the multi-table launch is off by default until it has been measured (csrc/walk_plan.h: kDfaMultiDefault): these tests ask for it"""
    monkeypatch.setenv("MFA_MIXED_DFA", "1")


def golden(auto):
    strings, bits = [], []
    for sset in auto["sets"]:
        strings += oracle_lib.load_set(sset)
        bits.append(oracle_lib.load_bits(auto["name"], sset))
    return strings, np.concatenate(bits)


def test_one_memoryless_image():
    """an object over one memory-less image is created and matched (before memory-less automata were accepted: ERR_UNSUPPORTED)"""
    auto = next(a for a in NFA if a["name"] == "nfa_abb_thompson")
    strings, want = golden(auto)
    mixed = capi.Mixed([capi.Image(fixture_blob(auto["name"]))])
    got = mixed_match(mixed, [strings])
    assert np.array_equal(got, want)
    assert mixed.last_launches()["region_launches"] == 0 and mixed.last_launches()["walk_launches"] == 0
    assert mixed.last_dfa()["own_launches"] == 1
    mixed.close()


def test_both_kinds_interleaved(monkeypatch):
    """all 26 memory-less fixtures and ten memory fixtures, interleaved, their golden sets as segments"""
    assert len(NFA) == 26 and len(MEM) == 10
    order, mem = [], list(MEM)
    for k, a in enumerate(NFA):
        order.append(a)
        if k % 3 == 1 and mem:
            order.append(mem.pop(0))
    order += mem
    assert len(order) == 36
    segments, wants = [], []
    for a in order:
        s, w = golden(a)
        segments.append(s); wants.append(w)
    want = np.concatenate(wants)
    n_dfa_strings = sum(len(s) for a, s in zip(order, segments) if a["name"].startswith("nfa_"))
    answers = {}
    for walk in ("table", "jit"):
        monkeypatch.setenv("MFA_WALK", walk)
        for multi in ("1", "0"):
            monkeypatch.setenv("MFA_MIXED_DFA", multi)
            mixed = capi.Mixed([capi.Image(fixture_blob(a["name"])) for a in order])
            got = mixed_match(mixed, segments)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, "MFA_WALK=%s MFA_MIXED_DFA=%s: %d mismatches, first string %d want %d got %d" % (walk, multi, bad.size, bad[0], want[bad[0]], got[bad[0]])
            d = mixed.last_dfa()
            if walk == "table" and multi == "1":
                assert d == {"multi_launches": 1, "own_launches": 0, "items": 26, "strings": n_dfa_strings}
            else:
                assert d["multi_launches"] == 0 and d["own_launches"] == 26
            assert mixed.last_launches()["region_launches"] >= 1
            answers[(walk, multi)] = got
            mixed.close()
    assert all(np.array_equal(v, answers[("table", "1")]) for v in answers.values())


def test_default_is_a_launch_per_segment(monkeypatch):
    monkeypatch.delenv("MFA_MIXED_DFA")
    autos = NFA[3:7]
    mixed = capi.Mixed([capi.Image(fixture_blob(a["name"])) for a in autos])
    got = mixed_match(mixed, [golden(a)[0] for a in autos])
    assert np.array_equal(got, np.concatenate([golden(a)[1] for a in autos]))
    assert mixed.last_dfa() == {"multi_launches": 0, "own_launches": 4, "items": 0, "strings": 0}
    mixed.close()


def test_memoryless_only_object():
    autos = NFA[:9]
    imgs = [capi.Image(fixture_blob(a["name"])) for a in autos]
    segments = [golden(a)[0] for a in autos]
    mixed = capi.Mixed(imgs)
    got = mixed_match(mixed, segments)
    assert mixed.last_launches()["region_launches"] == 0 and mixed.last_launches()["walk_launches"] == 0
    assert mixed.last_ms()[0] == 0.0 and mixed.last_ms()[1] > 0.0
    assert mixed.last_dfa()["multi_launches"] == 1 and mixed.last_dfa()["own_launches"] == 0
    want = np.concatenate([match_on_gpu(i, s)[0] for i, s in zip(imgs, segments)])
    assert np.array_equal(got, want) and np.array_equal(got, np.concatenate([golden(a)[1] for a in autos]))
    mixed.close()


def test_directions_mixed_in_one_object():
    rng = np.random.default_rng(3)
    strings = [bytes(rng.choice(list(b"ab"), size=int(n)).tolist()) + (b"abb" if k % 2 else b"") for k, n in enumerate(rng.integers(0, 900, size=700))]
    blobs = [fixture_blob("nfa_abb_glushkov", 0), fixture_blob("nfa_abb_glushkov", 1), fixture_blob("nfa_third_thompson", 1), fixture_blob("nfa_third_thompson", 0)]
    imgs = [capi.Image(b) for b in blobs]
    assert [i.info()["is_reversed"] for i in imgs] == [0, 1, 1, 0]
    segments = [strings, strings, strings[:300], strings[300:]]
    mixed = capi.Mixed(imgs)
    got = mixed_match(mixed, segments)
    assert mixed.last_dfa()["multi_launches"] == 1 and mixed.last_dfa()["items"] == 4
    want = np.concatenate([match_on_gpu(i, s)[0] for i, s in zip(imgs, segments)])
    assert np.array_equal(got, want)
    assert np.array_equal(got, np.concatenate([oracle_lib.OracleImage(b).match(s) for b, s in zip(blobs, segments)]))
    n = len(strings)
    assert not np.array_equal(got[:n], got[n:2 * n]) and 0 < got[:n].sum() < n       # the direction matters on these strings
    mixed.close()


def test_ineligible_image_beside_eligible_ones(tmp_path):
    """a table that does not fit LDS (hundreds of state sets: the Thompson image of (a|b)*a(a|b)^8) gets a launch of its own"""
    big = front_end_blob("(a|b)*a" + "(a|b)" * 8, tmp_path)
    blobs = [fixture_blob("nfa_abb_plain"), big, fixture_blob("nfa_enum_ssnf"), fixture_blob("ex1_plain")]
    imgs = [capi.Image(b) for b in blobs]
    assert imgs[1].info()["dfa_states"] > 127
    rng = np.random.default_rng(99)
    strings = [bytes(rng.choice(list(b"ab"), size=int(n)).tolist()) for n in rng.integers(0, 300, size=600)] + [b"", b"a" + b"b" * 8, b"b" * 9]
    segments = [strings, strings, strings[:200], strings[100:400]]
    mixed = capi.Mixed(imgs)
    got = mixed_match(mixed, segments)
    d = mixed.last_dfa()
    assert d["own_launches"] == 1 and d["multi_launches"] == 1 and d["items"] == 2
    want = np.concatenate([oracle_lib.OracleImage(b).match(s) for b, s in zip(blobs, segments)])
    assert np.array_equal(got, want) and 0 < want.sum() < len(want)
    mixed.close()


def test_edge_cases():
    import torch
    blobs = [fixture_blob("nfa_abb_thompson"), fixture_blob("ex1_plain"), fixture_blob("nfa_star2_plain"), fixture_blob("nfa_abb_glushkov", 1),
             fixture_blob("nfa_enum_glushkov"), fixture_blob("nfa_third_plain")]
    oracles = [oracle_lib.OracleImage(b) for b in blobs]
    mixed = capi.Mixed([capi.Image(b) for b in blobs])
    rng = np.random.default_rng(41)
    ragged = [bytes(rng.choice(list(b"ab"), size=int(n)).tolist()) for n in rng.integers(0, 70, size=400)]
    # empty segments at the start, in the middle and at the end; empty strings; a segment of one string
    segments = [[], [b"aa", b"", b"aaa"], [b"", b"a", b"", b"ba"], [], [b"abc"], []]
    want = np.concatenate([o.match(s) if s else np.zeros(0, dtype=np.uint8) for o, s in zip(oracles, segments)])
    assert np.array_equal(mixed_match(mixed, segments), want)
    assert mixed.last_dfa()["items"] == 2
    # strings that start and end at every residue mod 16
    segments = [ragged, ragged[:50], ragged[50:], ragged[::-1], [], ragged[:1]]
    strings = [s for seg in segments for s in seg]
    off = np.cumsum([0] + [len(s) for s in strings])
    assert {int(o) % 16 for o in off[:-1]} == set(range(16)) and {int(o) % 16 for o in off[1:]} == set(range(16))
    want = np.concatenate([o.match(s) if s else np.zeros(0, dtype=np.uint8) for o, s in zip(oracles, segments)])
    assert np.array_equal(mixed_match(mixed, segments), want)
    # a 1 MiB string in a small memory-less segment (walked whole by its lane): nfa_abb accepts ...abb
    long_ok, long_no = b"ab" * (1 << 19) + b"abb", b"ab" * (1 << 19) + b"ab"
    segments = [[b"abb", long_ok, b"ab", long_no], [b"aa"], [b"a"], [b"bba", long_ok[::-1]], [], []]
    got = mixed_match(mixed, segments)
    assert list(got) == [1, 1, 0, 0, 1, 1, 1, 1]
    # exactly MFA_MAX_STRING_BYTES is walked, one byte more is answered 2 (device buffers built on the device: 32 MiB of a, then abb)
    big = torch.full((2 * MAX_BYTES + 64 + 16,), ord("a"), dtype=torch.uint8, device="cuda")
    big[MAX_BYTES - 2:MAX_BYTES] = ord("b")                       # string 0 = a...abb, exactly at the limit
    d_off = torch.tensor([0, MAX_BYTES, 2 * MAX_BYTES + 1, 2 * MAX_BYTES + 4], dtype=torch.int64, device="cuda")
    big[2 * MAX_BYTES + 1:2 * MAX_BYTES + 4] = torch.tensor(list(b"abb"), dtype=torch.uint8, device="cuda")
    res = filled(3)
    mixed.match_tensors(big, d_off, [0, 3, 3, 3, 3, 3, 3], res)
    torch.cuda.synchronize()
    assert list(res[:3].cpu().numpy()) == [1, 2, 1]
    mixed.close()


def _two_batches():
    rng = np.random.default_rng(8)
    names = ["nfa_abb_thompson", "ex1_plain", "nfa_star1_plain", "nfa_enum_glushkov"]
    blobs = [fixture_blob(n) for n in names]
    batches = []
    for k in range(2):
        tails = [b"abb", b"", b"ab", b"abc"]
        segments = [[bytes(rng.choice(list(b"ab"), size=int(n)).tolist()) + (tails[j] if i % 2 else b"") for i, n in enumerate(rng.integers(0, 200 + 300 * k, size=500 + 40 * j + 333 * k))]
                    for j in range(4)]
        want = np.concatenate([oracle_lib.OracleImage(b).match(s) for b, s in zip(blobs, segments)])
        batches.append((segments, want))
        first = len(segments[0])
        assert 0 < want[:first].sum() < first and 0 < want[-len(segments[3]):].sum() < len(segments[3])
    assert len(batches[0][1]) != len(batches[1][1])
    return blobs, batches


def test_forty_alternating_calls_without_synchronising():
    import torch
    blobs, batches = _two_batches()
    mixed = capi.Mixed([capi.Image(b) for b in blobs])
    dev = []
    for segments, want in batches:
        strings = [s for seg in segments for s in seg]
        d_bytes, d_off, _ = upload(strings)
        dev.append((d_bytes, d_off, seg_first_of(segments), len(strings)))
    for streams in ([torch.cuda.current_stream()], [torch.cuda.Stream(), torch.cuda.Stream()]):
        results = [filled(dev[k % 2][3]) for k in range(40)]
        torch.cuda.synchronize()
        for k in range(40):
            d_bytes, d_off, sf, _ = dev[k % 2]
            mixed.match_tensors(d_bytes, d_off, sf, results[k], stream=streams[k % len(streams)])
        torch.cuda.synchronize()
        for k in range(40):
            assert np.array_equal(results[k].cpu().numpy(), batches[k % 2][1]), "call %d on %d stream(s)" % (k, len(streams))
    mixed.close()


def test_capture_and_replay():
    import torch
    blobs, batches = _two_batches()
    segments, want = batches[1]
    strings = [s for seg in segments for s in seg]
    d_bytes, d_off, _ = upload(strings)
    total = sum(len(s) for s in strings)
    res = filled(len(strings))
    mixed = capi.Mixed([capi.Image(b) for b in blobs])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        mixed.match_tensors(d_bytes, d_off, seg_first_of(segments), res, total_bytes=total)      # warm-up: tables, workspaces
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy(), want) and mixed.last_dfa()["multi_launches"] == 1
    res.fill_(7)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        mixed.match_tensors(d_bytes, d_off, seg_first_of(segments), res, total_bytes=total)
    torch.cuda.synchronize()
    for _ in range(2):
        res.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(res.cpu().numpy(), want)
    mixed.close()


def test_cli_match_mixed_with_flags(tmp_path):
    """`diploma -match-mixed -bnf FILE...` on regexes with and without backreferences prints what `diploma -match -bnf` prints per file;
    without a flag the command answers as before (every regex a memory automaton): the goldens' answers, nothing else"""
    names = ["ex1_bnf", "nfa_abb_plain", "ex5_bnf", "nfa_enum_plain", "nfa_star4_plain", "ex2_bnf"]
    files, per_file, plain_want = [], b"", []
    for name in names:
        auto = next(a for a in MANIFEST["automata"] if a["name"] == name)
        keep = [k for k, s in enumerate(oracle_lib.load_set("rnd")) if s and b"\n" not in s][:300]
        strings = [oracle_lib.load_set("rnd")[k] for k in keep]
        path = tmp_path / (name + ".txt")
        path.write_bytes(auto["regex"].encode() + b"\n" + b"".join(s + b"\n" for s in strings))
        files.append(str(path))
        p = subprocess.run([DIPLOMA, "-match", "-bnf"], input=auto["regex"].encode() + b"\n" + b"\n".join(strings) + b"\nexit\n", capture_output=True, cwd=tmp_path)
        assert p.returncode == 0, p.stderr
        per_file += p.stdout
        bits = oracle_lib.load_bits(name if name.startswith("nfa_") else name.split("_")[0] + "_plain", "rnd")
        plain_want += [int(bits[k]) for k in keep]
    p = subprocess.run([DIPLOMA, "-match-mixed", "-bnf"] + files, capture_output=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    assert p.stdout == per_file
    assert len(p.stdout.split(b"\n")) > 6 * 300
    # without a flag: 0/1 lines only, the language of each regex (the plain fixtures' goldens)
    p = subprocess.run([DIPLOMA, "-match-mixed"] + files, capture_output=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    assert p.stdout == b"".join(b"%d\n" % b for b in plain_want)
