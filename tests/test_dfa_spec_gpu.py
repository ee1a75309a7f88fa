"""Long strings of memory-less automata whose table lives in L2 (255 state sets and more) on the GPU: csrc/dfa_spec.hip cuts a string of
MFA_DFA_SPLIT_MIN bytes or more into chunks, walks every chunk from a guessed state, repairs wrong guesses in a fixed number of rounds and
resolves the rest exactly.  Answers against the CPU restatement and against the same call with MFA_DFA_SPEC=0; what the path did through
mfa_last_dfa_split and mfa_last_dfa_spec.  Tables of tests/test_dfa_spec_cpu.py (tests/testlib.py: TABLES)."""
import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi
from testlib import (CHUNK_MIN, DEAD, INVALID, SPLIT_MIN, START, check, expected_split, feed, filled, fixture_blob, front_end_blob, match_on_gpu, mixed_match,
                     new_states, rnd, short_strings, states_of, table_blob, upload)

pytestmark = pytest.mark.gpu

SMALL_MIN, SMALL_CHUNK = 256, 64


def prime(img):
    """A launch workspace of an L2-table image starts quiet: its first batch with a long string is walked whole by the main kernel, which tells
    the workspace, and from the next call on (same stream) long strings are cut.  One such batch, checked to have been walked whole."""
    got, _ = match_on_gpu(img, [b"ab" * 40000, b"ab"])
    assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)
    return got


def small_knobs(monkeypatch):
    monkeypatch.setenv("MFA_DFA_SPLIT_MIN", str(SMALL_MIN))
    monkeypatch.setenv("MFA_DFA_CHUNK", str(SMALL_CHUNK))


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("states", [514, 32770, 131074])
def test_small_knob_parity(states, rev, tmp_path, monkeypatch):
    """MFA_DFA_SPLIT_MIN=256, chunks of 64 bytes: 300 strings of 0 to 3 000 bytes and the edge strings of
    test_dfa_resume_gpu.py::test_every_table_form, on tables of 514, 32 770 (16-bit entries) and 131 074 (32-bit entries) state sets"""
    small_knobs(monkeypatch)
    k = {514: 8, 32770: 14, 131074: 16}[states]
    blob = front_end_blob("(a|b)*a" + "(a|b)" * k, tmp_path, rev)
    rng = np.random.default_rng(states + rev)
    strings = [rnd(b"ab", int(ln), rng) for ln in rng.integers(0, 3001, size=300)]
    strings += [b"", b"a" + b"b" * k, b"b" * (k + 1), b"ab" * 300 + b"a" + b"b" * k, b"ab" * 300 + b"b" + b"a" * k, b"abc" + b"a" * 30]
    if rev:
        strings = [s[::-1] for s in strings]
    img = capi.Image(blob)
    assert img.info()["dfa_states"] == states and img.info()["is_reversed"] == rev
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < want.sum() < len(strings)
    prime(img)
    got, off = match_on_gpu(img, strings)
    check(got, want, strings, "%d state sets, rev %d" % (states, rev))
    n_long, chunks, chunk = img.last_dfa_split()
    print("split", (n_long, chunks, chunk), "spec", img.last_dfa_spec())
    assert n_long > 0 and chunks > n_long
    assert (n_long, chunks, chunk) == expected_split(off, SMALL_MIN, SMALL_CHUNK)
    assert img.last_dfa_spec()[1:] == (0, 0)                  # the state is the last k + 1 bytes: 256 bytes of lookback make every guess right
    monkeypatch.setenv("MFA_DFA_SPEC", "0")
    plain, _ = match_on_gpu(img, strings)
    assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)
    check(got, plain, strings, "against the same call without the path")


def test_default_knobs(tmp_path):
    """the library's defaults: two strings of 1 MiB + 3 and 1 MiB - 1 bytes among five short ones on the 514-state image are cut from the
    workspace's second call on (before this path existed a table in L2 reported 0 strings on every call) and nothing is left to the serial walk"""
    blob = front_end_blob("(a|b)*a" + "(a|b)" * 8, tmp_path, 0)
    rng = np.random.default_rng(514)
    body = rnd(b"ab", (1 << 20) + 3, rng)
    strings = [b"ab", body[:-9] + b"a" + b"b" * 8, b"", b"a" + b"b" * 8, body[:(1 << 20) - 10] + b"b" + b"a" * 8, rnd(b"ab", 999, rng), b"b" * 9]
    assert [len(s) for s in strings if len(s) > 999] == [(1 << 20) + 3, (1 << 20) - 1]
    want = oracle_lib.OracleImage(blob).match(strings)
    assert (want[1], want[4]) == (1, 0)
    img = capi.Image(blob)
    assert img.info()["dfa_states"] == 514
    got, off = match_on_gpu(img, strings)                         # a fresh workspace: walked whole this once, and right
    check(got, want, strings, "default knobs, first call")
    assert img.last_dfa_split() == (0, 0, 0)
    got, off = match_on_gpu(img, strings)
    check(got, want, strings, "default knobs")
    print("split", img.last_dfa_split(), "spec", img.last_dfa_spec())
    assert img.last_dfa_split() == expected_split(off, SPLIT_MIN, CHUNK_MIN) and img.last_dfa_split()[0] == 2
    assert img.last_dfa_spec()[1] == 0
    assert img.info()["last_kernel"] == capi.KERNEL_TABLE


@pytest.mark.parametrize("rounds", [0, 3])
@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("name", ["counter", "prefix"])
def test_tables_that_guess_badly(name, rev, rounds, tmp_path, monkeypatch):
    """(a^300)*, whose state is a position modulo 300 and never converges: the resolve step has to walk serially, and the answers are exact;
    a literal prefix in front of the 514-state regex, on which the first seed of every guess dies: parity (what repairing cost is printed)"""
    small_knobs(monkeypatch)
    monkeypatch.setenv("MFA_DFA_SPEC_ROUNDS", str(rounds))
    blob = table_blob(name, tmp_path, rev)
    rng = np.random.default_rng(len(name) + rev)
    if name == "counter":
        strings = [b"a" * n for n in (3000, 2999, 150, 300, 256, 257, 4500, 4501, 0, 1, 1500)] + [b"a" * 1000 + b"b" + b"a" * 499, b"a" * 40]
    else:
        strings = [b"xyz" + rnd(b"ab", int(n), rng) for n in rng.integers(0, 3000, size=60)] + [rnd(b"ab", 2000, rng), b"xy", b"", b"xyz" + b"a" + b"b" * 8]
    if rev:
        strings = [s[::-1] for s in strings]
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < want.sum() < len(strings)
    img = capi.Image(blob)
    assert img.info()["dfa_states"] >= 255
    prime(img)
    got, off = match_on_gpu(img, strings)
    check(got, want, strings, "%s rev %d rounds %d" % (name, rev, rounds))
    assert img.last_dfa_split() == expected_split(off, SMALL_MIN, SMALL_CHUNK)
    rewalked, serial_strings, serial_bytes = img.last_dfa_spec()
    print(name, "rev", rev, "rounds", rounds, "rewalked", rewalked, "serial strings", serial_strings, "serial bytes", serial_bytes)
    if rounds == 0:
        assert rewalked == 0
    if name == "counter":
        assert serial_strings > 0 and serial_bytes > 0


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
def test_resume_pieces_through_the_path(rev, tmp_path, monkeypatch):
    """strings cut in two: the second halves are pieces of MFA_DFA_SPLIT_MIN bytes or more entered from states that are not START.  Among
    them a word that enters dead (stays dead, bytes not read) and an invalid word (sticky, result 2), neither cut.  States and results are
    those of one call on the whole strings, also when the first round has no result bytes."""
    small_knobs(monkeypatch)
    blob = front_end_blob("(a|b)*a" + "(a|b)" * 8, tmp_path, rev)
    rng = np.random.default_rng(77 + rev)
    strings = [rnd(b"ab", int(n), rng) for n in (2000, 3001, 600, 5000, 513, 40, 0, 1024, 2047)]
    if rev:
        strings = [s[::-1] for s in strings]
    halves = [(s[len(s) // 2:], s[:len(s) // 2]) if rev else (s[:len(s) // 2], s[len(s) // 2:]) for s in strings]       # scan order
    img = capi.Image(blob)
    n = len(strings)
    prime(img)
    whole_states = new_states(n)
    whole = feed(img, strings, whole_states)
    check(whole, oracle_lib.OracleImage(blob).match(strings), strings, "whole strings, rev %d" % rev)
    assert img.last_dfa_split()[0] == sum(len(s) >= SMALL_MIN for s in strings)
    for with_results in (True, False):
        d_states = new_states(n)
        assert (feed(img, [h[0] for h in halves], d_states, results=with_results) is not None) == with_results
        mid = states_of(d_states, n)
        assert all(st not in (DEAD, INVALID) for st in mid) and sum(st != START for st, h in zip(mid, halves) if len(h[1]) >= SMALL_MIN) >= 3
        got = feed(img, [h[1] for h in halves], d_states)
        assert img.last_dfa_split()[0] == sum(len(h[1]) >= SMALL_MIN for h in halves) > 0
        assert np.array_equal(states_of(d_states, n), states_of(whole_states, n)) and np.array_equal(got, whole)
    # dead and invalid words in front of long pieces
    import torch
    words = np.array([DEAD, INVALID, START, img.info()["dfa_states"]], dtype=np.uint32)
    d_states = torch.from_numpy(words.view(np.int32)).cuda()
    pieces = [strings[0], strings[1], strings[0], strings[3]]
    got = feed(img, pieces, d_states)
    assert img.last_dfa_split()[0] == 1                       # only the word that walks is queued
    st = states_of(d_states, 4)
    assert list(got) == [0, 2, whole[0], 2] and list(st[:2]) == [DEAD, INVALID] and st[2] == states_of(whole_states, n)[0] and st[3] == INVALID


def path_off_corpus(rev, seed):
    """the 514-state image, about 60 strings of 0 to 3 000 bytes and the edge strings of test_small_knob_parity"""
    k = 8
    rng = np.random.default_rng(seed + rev)
    strings = [rnd(b"ab", int(ln), rng) for ln in rng.integers(0, 3001, size=60)]
    strings += [b"", b"a" + b"b" * k, b"b" * (k + 1), b"ab" * 300 + b"a" + b"b" * k, b"ab" * 300 + b"b" + b"a" * k, b"abc" + b"a" * 30]
    if rev:
        strings = [s[::-1] for s in strings]
    return strings, rng


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
def test_resume_with_the_path_off(rev, tmp_path, monkeypatch):
    """MFA_DFA_SPEC=0 on a resume call: the same main kernel with the queue off.  Every string in three pieces (scan order), once with the
    path and once without: final states and result bytes are equal, the results are the oracle's on the whole strings, the second run
    reports no cut string.  A word that enters dead and an invalid word, both in front of long pieces, leave as they came (results 0 and 2)."""
    import torch
    small_knobs(monkeypatch)
    blob = front_end_blob("(a|b)*a" + "(a|b)" * 8, tmp_path, rev)
    strings, rng = path_off_corpus(rev, 41)
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < want.sum() < len(strings)
    strings += [rnd(b"ab", 2000, rng), rnd(b"ab", 2500, rng)]              # entered dead, entered invalid
    n = len(strings)
    rounds = [[], [], []]
    for s in strings:
        a, b = sorted(int(x) for x in rng.integers(0, len(s) + 1, size=2))
        parts = [s[:a], s[a:b], s[b:]]
        for r, part in enumerate(parts[::-1] if rev else parts):
            rounds[r].append(part)
    words = np.full(n, START, dtype=np.uint32)
    words[-2:] = (DEAD, INVALID)
    img = capi.Image(blob)
    assert img.info()["dfa_states"] == 514 and img.info()["is_reversed"] == rev
    prime(img)
    runs = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("MFA_DFA_SPEC", "0")
        d_states = torch.from_numpy(words.view(np.int32).copy()).cuda()
        cut = 0
        for r in range(3):
            got = feed(img, rounds[r], d_states)
            cut += img.last_dfa_split()[0]
            if off:
                assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)
            assert list(got[-2:]) == [0, 2] and list(states_of(d_states, n)[-2:]) == [DEAD, INVALID]
        assert (cut == 0) == off                               # with the path, pieces of 256 bytes and more were cut
        runs.append((states_of(d_states, n), got))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    check(runs[1][1][:-2], want, strings, "three pieces without the path, rev %d" % rev)
    whole_states = new_states(n - 2)
    feed(img, strings[:-2], whole_states)
    assert np.array_equal(runs[1][0][:-2], states_of(whole_states, n - 2))


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
def test_plain_call_with_the_split_off(rev, tmp_path, monkeypatch):
    """MFA_DFA_SPLIT=0 on mfa_match_batch, on a workspace that would cut otherwise: the same main kernel with the queue off"""
    small_knobs(monkeypatch)
    blob = front_end_blob("(a|b)*a" + "(a|b)" * 8, tmp_path, rev)
    strings, _ = path_off_corpus(rev, 43)
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < want.sum() < len(strings)
    img = capi.Image(blob)
    assert img.info()["dfa_states"] == 514
    prime(img)
    monkeypatch.setenv("MFA_DFA_SPLIT", "0")
    got, off = match_on_gpu(img, strings)
    check(got, want, strings, "MFA_DFA_SPLIT=0, rev %d" % rev)
    assert expected_split(off, SMALL_MIN, SMALL_CHUNK)[0] > 0
    assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)


def test_quiet_workspace_hands_long_strings_over(tmp_path):
    """the cycle of test_dfa_split_gpu.py::test_quiet_workspace_hands_long_strings_over on the 514-state image: quiet calls drop the extra
    launches, the first long batch after that is walked whole by the main kernel and still right, then the tail comes back for good"""
    blob = front_end_blob("(a|b)*a" + "(a|b)" * 8, tmp_path, 0)
    rng = np.random.default_rng(31)
    ora = oracle_lib.OracleImage(blob)
    short = short_strings(rng)
    longs = short[:40] + [rnd(b"ab", 200000, rng), rnd(b"ab", 65536, rng), b"", rnd(b"ab", 65535, rng)] + short[40:90]
    want_short, want_long = ora.match(short), ora.match(longs)
    img = capi.Image(blob)
    for call in range(8):                                      # quiet after four calls that reported no long string
        got, _ = match_on_gpu(img, short)
        check(got, want_short, short, "short batch, call %d" % call)
        assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)
    got, off = match_on_gpu(img, longs)
    check(got, want_long, longs, "long strings in a call without the tail")
    assert img.last_dfa_split() == (0, 0, 0)                   # walked whole, this once
    cut = expected_split(off, SPLIT_MIN, CHUNK_MIN)
    assert cut[0] == 2
    for round_ in range(2):
        got, _ = match_on_gpu(img, longs)
        check(got, want_long, longs, "long strings again")
        assert img.last_dfa_split() == cut
        for call in range(6):
            got, _ = match_on_gpu(img, short)
            check(got, want_short, short, "short batch after long ones")
            assert img.last_dfa_split() == (0, 0, 0)


def test_call_is_capturable(tmp_path):
    """after a first call with long strings the call is captured (one stream, no parallel branches: the launch count is fixed at enqueue time)
    and replayed on new bytes of the same lengths"""
    import torch
    blob = front_end_blob("(a|b)*a" + "(a|b)" * 8, tmp_path, 0)
    rng = np.random.default_rng(12)
    lens = [300000, 2, 150001, 9, 0]
    first = [rnd(b"ab", ln, rng) for ln in lens]
    second = [rnd(b"ab", ln, rng) for ln in lens]
    second[0] = second[0][:-9] + b"a" + b"b" * 8
    second[2] = second[2][:-9] + b"b" + b"a" * 8
    ora = oracle_lib.OracleImage(blob)
    want_first, want_second = ora.match(first), ora.match(second)
    d_bytes, d_off, off = upload(first)
    res = filled(len(lens))
    img = capi.Image(blob)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        img.match_tensors(d_bytes, d_off, res)                 # this stream's workspace meets long strings: walked whole
        torch.cuda.synchronize()
        assert np.array_equal(res.cpu().numpy(), want_first) and img.last_dfa_split() == (0, 0, 0)
        img.match_tensors(d_bytes, d_off, res)                 # cut: allocates the arena
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy(), want_first) and img.last_dfa_split()[0] == 2
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        img.match_tensors(d_bytes, d_off, res)
    torch.cuda.synchronize()
    for strings, want in ((first, want_first), (second, want_second)):
        data, _ = oracle_lib.pack(strings)
        d_bytes[:len(data)] = torch.from_numpy(data.copy()).cuda()
        res.fill_(7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(res.cpu().numpy(), want)


def test_in_a_mixed_batch(tmp_path, monkeypatch):
    """a mixed object with the 514-state image beside nfa_abb_plain and ex1_plain: the L2 segment gets a launch of its own, its long string is cut"""
    small_knobs(monkeypatch)
    blobs = [fixture_blob("nfa_abb_plain"), front_end_blob("(a|b)*a" + "(a|b)" * 8, tmp_path, 0), fixture_blob("ex1_plain")]
    imgs = [capi.Image(b) for b in blobs]
    rng = np.random.default_rng(99)
    strings = [rnd(b"ab", int(n), rng) for n in rng.integers(0, 200, size=300)] + [b"", b"a" + b"b" * 8, b"b" * 9]
    long_one = rnd(b"ab", 3000, rng) + b"a" + b"b" * 8
    segments = [strings, strings[:100] + [long_one] + strings[100:], strings[:200]]
    mixed = capi.Mixed(imgs)
    first = mixed_match(mixed, segments)                       # the mixed object's stream is a workspace of its own: walked whole this once
    assert imgs[1].last_dfa_split() == (0, 0, 0)
    got = mixed_match(mixed, segments)
    assert np.array_equal(first, got)
    want = np.concatenate([oracle_lib.OracleImage(b).match(s) for b, s in zip(blobs, segments)])
    assert np.array_equal(got, want) and want[len(strings) + 100] == 1
    assert mixed.last_dfa()["own_launches"] >= 1
    assert imgs[1].last_dfa_split()[0] == 1 and imgs[1].last_dfa_spec()[1] == 0
    mixed.close()
