"""Long strings of set-walk images cut across the GPU (csrc/nfa_set_split.hip behind the main kernels of csrc/nfa_set.hip): mfa_match_batch and
mfa_match_batch_resume_set against the CPU restatement and, record for record, against the host harness of the whole walk
(tests/emul/nfa_set_resume_emul.cpp); the counts of mfa_last_set_split against the host harness of the split path
(tests/emul/nfa_set_split_emul.cpp, which tests/test_nfa_set_split_cpu.py holds to the whole walk).  Small shapes: MFA_DFA_SPLIT_MIN=1024,
MFA_DFA_CHUNK=64, strings of 1 to 5 KiB."""
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi, image
from setwalk_lib import (COUNTER, INVALID, LANE_WORDS, LIVE, PREFIX, ab_strings, feed_records, k_blob, new_records, record, records_of, records_view, run_lane_pieces,
                         run_lane_split)
from testlib import DIPLOMA, MAX_BYTES, blob_of, emul_exe, expected_split, filled, front_end_blob, manifest_entry, match_on_gpu, mixed_match, rnd, upload, wide_images

pytestmark = pytest.mark.gpu

SPLIT_MIN, CHUNK = 1024, 64
KNOBS = ("MFA_NFA_SETWALK", "MFA_DFA_STATE_LIMIT", "MFA_DFA_SPLIT", "MFA_DFA_SPLIT_MIN", "MFA_DFA_CHUNK", "MFA_DFA_ARENA", "MFA_SET_SPLIT", "MFA_SET_SPLIT_ROUNDS",
         "MFA_SET_SPLIT_LOOKBACK")


@pytest.fixture()
def env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MFA_DFA_SPLIT_MIN", str(SPLIT_MIN))
    monkeypatch.setenv("MFA_DFA_CHUNK", str(CHUNK))
    return monkeypatch


def forced(env, blob):
    """the blob's image as a set-walk image, whatever its number of state sets"""
    env.setenv("MFA_NFA_SETWALK", "1")
    img = capi.Image(blob)
    env.delenv("MFA_NFA_SETWALK")
    assert img.info()["dfa_states"] == 0
    return img


def mismatch(got, want, strings, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d mismatches, first string %d (len %d) want %d got %d" % (what, bad.size, bad[0], len(strings[bad[0]]), want[bad[0]], got[bad[0]])


def ragged_batch(alpha, rng, tail=b""):
    """lengths split_min - 1, split_min, split_min + 1 and around chunk multiples up to 5 KiB, between short and empty strings that put them
    at unaligned offsets; every long length once with `tail` at its end"""
    longs = [SPLIT_MIN - 1, SPLIT_MIN, SPLIT_MIN + 1, 17 * CHUNK - 1, 17 * CHUNK, 17 * CHUNK + 1, 32 * CHUNK - 1, 32 * CHUNK, 32 * CHUNK + 1, 3000, 5 * 1024]
    out = []
    for k, ln in enumerate(longs + longs):
        out.append(rnd(alpha, int(rng.integers(0, 40)), rng) if k % 3 else b"")
        s = rnd(alpha, ln, rng)
        out.append(s[:ln - len(tail)] + tail if k >= len(longs) else s)
    return out + [b"", rnd(alpha, 7, rng)]


def check_split_report(img, off, what):
    n_long, chunks, chunk = expected_split(off, SPLIT_MIN, CHUNK)
    got = img.last_set_split()
    assert n_long > 0 and chunks > 0 and got[:3] == (n_long, chunks, chunk), (what, got)
    assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0) and img.last_kernel_ms() > 0.0
    assert img.info()["last_kernel"] == capi.KERNEL_NODESET
    return got


def test_every_width_and_both_directions(env, tmp_path):
    rng = np.random.default_rng(91)
    blobs = {("abb", 0): blob_of("nfa_abb_thompson", 0), ("abb", 1): blob_of("nfa_abb_thompson", 1)}
    ab = "(a|b)"
    regexes = {"w2": "(a|b)*a" + ab * 4 + "(c|(a|b))*", "w4": "((a|b)|(c|a))*" + "((a|b)|c)" * 6, "w8": "((a|b)|(c|a))*" + "((a|(b|c))|(c|(a|b)))" * 8}
    for key, rx in regexes.items():
        for rev in (0, 1):
            blobs[(key, rev)] = front_end_blob(rx, tmp_path, rev)
    blobs[("deep", 1)] = wide_images(tmp_path)["deep"]
    seen_w = set()
    for (key, rev), blob in blobs.items():
        img = forced(env, blob)
        strings = ragged_batch(b"ab" if key == "abb" else b"abc", rng, tail=b"abb" if key == "abb" else b"")
        if image.blob_info(blob)["reversed"]:
            strings = [s[::-1] for s in strings]
        want = oracle_lib.OracleImage(blob).match(strings)
        if key != "deep":
            assert 0 < int(want.sum()) < len(strings), key
        got, off = match_on_gpu(img, strings, exact=True)
        mismatch(got, want, strings, "%s rev %d" % (key, rev))
        assert sum(1 for o, s in zip(off, strings) if len(s) >= SPLIT_MIN and int(o) % 16) > 4      # long strings at unaligned offsets
        check_split_report(img, off, key)
        n_nodes = image.blob_info(blob)["n_nodes"]
        seen_w.add(1 if n_nodes <= 32 else 2 if n_nodes <= 64 else 4 if n_nodes <= 128 else 8)
    assert seen_w == {1, 2, 4, 8}


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
def test_resume_form(env, rev, tmp_path):
    """pieces in three rounds, long pieces cut: each round the records equal the whole-walk harness's word for word and the results the
    oracle's.  Dead and INVALID records are not queued and keep their answers"""
    emul = emul_exe("nfa_set_resume")
    rng = np.random.default_rng(17 + rev)
    blob = front_end_blob("(a|b)*a" + "(a|b)" * 4 + "(c|(a|b))*", tmp_path, rev)      # W = 2
    img = forced(env, blob)
    lens = [(1500, 1024, 2000), (40, 3000, 0), (1023, 1025, 64), (0, 5000, 1100), (1100, 1100, 1100), (5, 0, 1024), (2048, 10, 2049)]
    strings = [(rnd(b"ab", sum(t), rng)[:-30] + rnd(b"abc", 30, rng))[:sum(t)] for t in lens]      # (ab in front: no set dies, every long piece is queued)
    if rev:
        strings = [s[::-1] for s in strings]
    ora = oracle_lib.OracleImage(blob)
    rounds = []
    for r in range(3):
        row = []
        for s, t in zip(strings, lens):
            cuts = [0, t[0], t[0] + t[1], sum(t)]
            if rev:
                cuts = [0, t[2], t[2] + t[1], sum(t)]
                row.append((len(s) - cuts[r + 1], len(s) - cuts[r]))
            else:
                row.append((cuts[r], cuts[r + 1]))
        rounds.append(row)
    d_states = new_records(len(strings), LANE_WORDS)
    for r in range(3):
        pieces = [s[b:e] for s, (b, e) in zip(strings, rounds[r])]
        got = feed_records(img, pieces, d_states, LANE_WORDS)
        seen = [s[rounds[r][k][0]:] if rev else s[:rounds[r][k][1]] for k, s in enumerate(strings)]
        mismatch(got, ora.match(seen), seen, "round %d" % r)
        _, recs_host = run_lane_pieces(emul, tmp_path, blob, strings, rounds[:r + 1])
        assert np.array_equal(records_of(d_states, len(strings), LANE_WORDS), recs_host), "round %d" % r
        assert img.last_set_split()[0] == sum(1 for p in pieces if len(p) >= SPLIT_MIN) and img.last_dfa_split() == (0, 0, 0)
    # dead, INVALID and a live neighbour, each with a long piece: only the neighbour is queued
    rows = np.stack([record(LANE_WORDS, LIVE), record(LANE_WORDS, INVALID), record(LANE_WORDS, 0)])
    d_states = new_records(3, LANE_WORDS, rows)
    got = feed_records(img, [strings[1]] * 3, d_states, LANE_WORDS)
    recs = records_of(d_states, 3, LANE_WORDS)
    assert list(got[:2]) == [0, 2] and got[2] == ora.match([strings[1]])[0]
    assert list(recs[0]) == [LIVE] + [0] * 11 and list(recs[1]) == [INVALID] + [0] * 11 and recs[2, 0] == LIVE
    assert img.last_set_split()[0] == 1


def test_over_long_piece_is_not_queued(env):
    """a piece of MFA_MAX_STRING_BYTES + 1 bytes: sticky error as before, not queued; its long neighbour is cut"""
    import torch
    img = forced(env, blob_of("nfa_abb_thompson", 0))
    big = torch.full((MAX_BYTES + 1 + 2000 + 64,), ord("a"), dtype=torch.uint8, device="cuda")
    big[MAX_BYTES + 1 + 1997:MAX_BYTES + 1 + 2000] = torch.tensor(list(b"abb"), dtype=torch.uint8, device="cuda")
    d_off = torch.tensor([0, MAX_BYTES + 1, MAX_BYTES + 1 + 2000], dtype=torch.int64, device="cuda")
    d_states = new_records(2, LANE_WORDS)
    res = filled(2)
    img.match_tensors_resume_set(big, d_off, records_view(d_states, 2, LANE_WORDS), res)
    torch.cuda.synchronize()
    recs = records_of(d_states, 2, LANE_WORDS)
    assert list(res.cpu().numpy()) == [2, 1] and list(recs[0]) == [INVALID] + [0] * 11 and recs[1, 0] == LIVE
    assert img.last_set_split()[0] == 1


def test_default_knobs_cut_a_megabyte(env, tmp_path):
    """the library's own defaults on the k = 10 Thompson image under a tabulation limit of 1000: two strings of 1 MiB are cut and their
    chunks join up -- nothing is left to the serial walk"""
    for k in ("MFA_DFA_SPLIT_MIN", "MFA_DFA_CHUNK"):
        env.delenv(k)
    blob = k_blob(10, tmp_path)
    env.setenv("MFA_DFA_STATE_LIMIT", "1000")
    img = capi.Image(blob)
    env.delenv("MFA_DFA_STATE_LIMIT")
    assert img.info()["dfa_states"] == 0
    rng = np.random.default_rng(2)
    strings = [b"ab", rnd(b"ab", 1 << 20, rng), b"", rnd(b"ab", 1 << 20, rng)[:-11] + b"a" + b"b" * 10]
    want = oracle_lib.OracleImage(blob).match(strings)
    assert want[3] == 1
    got, _ = match_on_gpu(img, strings)
    mismatch(got, want, strings, "k = 10, default knobs")
    n_long, chunks, chunk, rewalked, serial_strings, serial_bytes = img.last_set_split()
    assert n_long == 2 and chunks >= 2 * (1 << 20) // chunk and chunk % 16 == 0 and (serial_strings, serial_bytes) == (0, 0)


def counts_against_the_harness(env, tmp_path, img, blob, strings, rounds, lookback=256):
    """one batch of long strings only: the answers are the oracle's and the counts of mfa_last_set_split those of the host harness on the same
    batch with the same settings (it cuts every string, so every string here is long)"""
    assert all(len(s) >= SPLIT_MIN for s in strings)
    env.setenv("MFA_SET_SPLIT_ROUNDS", str(rounds))
    env.setenv("MFA_SET_SPLIT_LOOKBACK", str(lookback))
    got, off = match_on_gpu(img, strings, exact=True)
    mismatch(got, oracle_lib.OracleImage(blob).match(strings), strings, "rounds %d" % rounds)
    report = check_split_report(img, off, "rounds %d" % rounds)
    (_, host, _), = run_lane_split(emul_exe("nfa_set_split"), tmp_path, blob, strings, (CHUNK,), (lookback,), (rounds,))
    assert report[3:] == (host["rewalked"], host["serial_strings"], host["serial_bytes"]), (report, host)
    return report, host


def test_counter_is_resolved_serially(env, tmp_path):
    """(a^250)*, the longest round counter a set-walk image holds: a position modulo 250 cannot be guessed, every long string is resolved
    serially at 0 and at 3 rounds, and the answers are right.  (Lengths are multiples of 16: the chunk grid starts at the string.)"""
    blob = front_end_blob(COUNTER, tmp_path)
    img = forced(env, blob)
    strings = [b"a" * 2000, b"a" * 2016, b"a" * 4000, b"a" * 3008, b"a" * 1600 + b"b" + b"a" * 399, b"a" * 4999]
    assert list(oracle_lib.OracleImage(blob).match(strings)) == [1, 0, 1, 0, 0, 0]
    r0, _ = counts_against_the_harness(env, tmp_path, img, blob, strings, 0)
    r3, _ = counts_against_the_harness(env, tmp_path, img, blob, strings, 3)
    assert r0[3] == 0 and r0[4] == len(strings) and r3[3] > 0 and r3[4] == len(strings) and 0 < r3[5] < r0[5]


def test_literal_prefix_guesses_the_home_set(env, tmp_path):
    """xyz(a|b)*abb: a walk from {start} dies on the text in front of every chunk, the home set's does not; behind a run of z both die and the
    guess is the home set itself.  Nothing of the accepted strings is left to the serial walk"""
    blob = front_end_blob(PREFIX, tmp_path)
    img = forced(env, blob)
    rng = np.random.default_rng(5)
    body = ab_strings([1500, 2048, 4000], rng, tail=b"abb")
    strings = [b"xyz" + s for s in body]
    report, host = counts_against_the_harness(env, tmp_path, img, blob, strings, 0, lookback=8)
    assert report[3:] == (0, 0, 0) and host["home_guesses"] == 0
    strings = strings + [b"xyz" + body[0][:300] + b"z" * 80 + body[0][300:], body[1]]
    for rounds in (0, 3):
        _, host = counts_against_the_harness(env, tmp_path, img, blob, strings, rounds, lookback=8)
        assert host["home_guesses"] > 0


def test_k_images_need_no_repair(env, tmp_path):
    """(a|b)*a(a|b)^8 under a limit that sends it to the set walk, lookback 256, 64-byte chunks: 0 chunks walked again, 0 strings resolved serially"""
    rng = np.random.default_rng(8)
    strings = ab_strings([1024, 1025, 2048, 3000, 5 * 1024], rng)
    for rev in (0, 1):
        blob = k_blob(8, tmp_path, rev)
        env.setenv("MFA_DFA_STATE_LIMIT", "100")
        img = capi.Image(blob)
        env.delenv("MFA_DFA_STATE_LIMIT")
        assert img.info()["dfa_states"] == 0
        report, _ = counts_against_the_harness(env, tmp_path, img, blob, strings, 3)
        assert report[3:] == (0, 0, 0)


@pytest.mark.parametrize("knob", ["MFA_SET_SPLIT", "MFA_DFA_SPLIT"])
def test_turned_off(env, knob):
    blob = blob_of("nfa_abb_thompson", 0)
    img = forced(env, blob)
    strings = ragged_batch(b"ab", np.random.default_rng(4), tail=b"abb")
    want = oracle_lib.OracleImage(blob).match(strings)
    on, _ = match_on_gpu(img, strings)
    assert img.last_set_split()[0] > 0
    env.setenv(knob, "0")
    off, _ = match_on_gpu(img, strings)
    mismatch(on, want, strings, "on")
    mismatch(off, want, strings, knob + "=0")
    assert img.last_set_split() == (0, 0, 0, 0, 0, 0) and img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)
    d_states = new_records(len(strings), LANE_WORDS)
    mismatch(feed_records(img, strings, d_states, LANE_WORDS), want, strings, knob + "=0, resume form")
    assert img.last_set_split() == (0, 0, 0, 0, 0, 0)


def test_queue_overflow(env):
    """16 400 strings of 1 040 bytes: 16 384 are queued and cut, the rest are walked by the main kernel, all answers are right"""
    blob = blob_of("nfa_abb_thompson", 0)
    img = forced(env, blob)
    rng = np.random.default_rng(6)
    kinds = [rnd(b"ab", 1037, rng) + (b"abb" if k % 2 else b"bab") for k in range(16)]
    want16 = oracle_lib.OracleImage(blob).match(kinds)
    assert list(want16) == [0, 1] * 8
    strings = [kinds[k % 16] for k in range(16400)]
    got, _ = match_on_gpu(img, strings)
    mismatch(got, np.tile(want16, 1025), strings, "queue overflow")
    n_long, chunks, chunk = img.last_set_split()[:3]
    assert n_long == 16384 and chunks > 0 and chunk >= CHUNK


def test_call_is_capturable(env):
    """after a first uncaptured call, one call is captured on one stream (no parallel branches) and replayed with new bytes in the same buffers"""
    import torch
    blob = blob_of("nfa_abb_thompson", 0)
    img = forced(env, blob)
    rng = np.random.default_rng(13)
    first = [rnd(b"ab", 3000, rng), b"ab", rnd(b"ab", 1021, rng) + b"abb", b"abb", b""]
    second = [rnd(b"ab", len(s), rng) for s in first]
    second[0] = second[0][:-3] + b"abb"
    ora = oracle_lib.OracleImage(blob)
    d_bytes, d_off, _ = upload(first)
    res = filled(len(first))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        img.match_tensors(d_bytes, d_off, res)                           # allocates the workspace, raises the kernels' LDS limit
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy(), ora.match(first)) and img.last_set_split()[0] == 2
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        img.match_tensors(d_bytes, d_off, res)
    torch.cuda.synchronize()
    for strings in (first, second):
        data, _ = oracle_lib.pack(strings)
        d_bytes[:len(data)] = torch.from_numpy(data.copy()).cuda()
        res.fill_(7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(res.cpu().numpy(), ora.match(strings))


def test_mixed_object_inherits_the_path(env):
    """a mixed object whose set-walk segment holds long strings answers what the per-image calls answer"""
    blobs = [blob_of("nfa_abb_thompson", 0), blob_of("nfa_star4_ssnf", 0)]
    sw, tab = forced(env, blobs[0]), capi.Image(blobs[1])
    assert tab.info()["dfa_states"] != 0
    rng = np.random.default_rng(21)
    segments = [ragged_batch(b"ab", rng, tail=b"abb"), [b"ab" * 40 + b"a", b"c" * 2000 + b"a", b"", b"abab" * 300 + b"a"]]
    mixed = capi.Mixed([sw, tab])
    got = mixed_match(mixed, segments)
    mixed.close()
    want = np.concatenate([oracle_lib.OracleImage(b).match(seg) for b, seg in zip(blobs, segments)])
    mismatch(got, want, segments[0] + segments[1], "mixed")
    assert sw.last_set_split()[0] == sum(1 for s in segments[0] if len(s) >= SPLIT_MIN)
    own = np.concatenate([match_on_gpu(sw, segments[0])[0], match_on_gpu(tab, segments[1])[0]])
    assert np.array_equal(got, own)


def test_cli_token_beyond_the_limit(env, tmp_path):
    """`diploma -match` on (a|b)*abb forced to the set walk, with tokens of 17 MiB -- one accepted, one rejected by its last byte: the host
    mirror feeds them in pieces through mfa_match_batch_resume_set_host, and the answers are the oracle's"""
    for k in ("MFA_DFA_SPLIT_MIN", "MFA_DFA_CHUNK"):
        env.delenv(k)
    env.setenv("MFA_NFA_SETWALK", "1")
    rng = np.random.default_rng(30)
    n = 17 << 20
    ok = rnd(b"ab", n - 3, rng) + b"abb"
    tokens = [b"aabb", ok, ok[:-1] + b"a", b"ab"]
    assert n > MAX_BYTES
    auto = manifest_entry("nfa_abb_plain")                               # (a|b)*abb as `diploma -match` compiles it
    want = oracle_lib.OracleImage(blob_of("nfa_abb_plain", 0)).match(tokens)
    assert list(want) == [1, 1, 0, 0]
    p = subprocess.run([DIPLOMA, "-match"], input=auto["regex"].encode() + b"\n" + b"\n".join(tokens) + b"\nexit\n", capture_output=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-400:]
    assert p.stdout == auto["header"].encode() + b"".join(b"%d\n" % w for w in want)
