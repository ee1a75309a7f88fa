"""Long strings of wave images cut across the GPU (csrc/nfa_set_wave_split.hip behind the main kernels of csrc/nfa_set_wave.hip):
mfa_match_batch and mfa_match_batch_resume_set_wide against the CPU restatement and, record for record, against the host harness of the
whole walk (tests/emul/nfa_set_wave_resume_emul.cpp); the counts of mfa_last_set_split against the host harness of the split path
(tests/emul/nfa_set_wave_split_emul.cpp, which tests/test_nfa_set_wave_split_cpu.py holds to the whole walk).  Small shapes:
MFA_DFA_SPLIT_MIN=1024, MFA_DFA_CHUNK=64, strings of at most 5 KiB."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from mfa_amd import capi, image
from setwalk_lib import (COUNTER300, INVALID, LANE_MAX_NODES, LIVE, PREFIX_WIDE, WIDE_WORDS, ab_strings, feed_records, new_records, pieces_of, raw_corpus_once, record, records_of,
                         results_of, run_wave_split, run_wide_pieces, tables_in_lds, wide_regex_images)
from testlib import DIPLOMA, blob_of, emul_exe, expected_split, filled, front_end_blob, match_on_gpu, mixed_match, rnd, upload

pytestmark = pytest.mark.gpu

SPLIT_MIN, CHUNK, ARENA = 1024, 64, 32768        # ARENA: the most chunks a wave image's workspace reserves (nfa_set_wave_split_core.h)
KNOBS = ("MFA_NFA_SETWALK", "MFA_DFA_STATE_LIMIT", "MFA_SET_WAVE", "MFA_DFA_SPLIT", "MFA_DFA_SPLIT_MIN", "MFA_DFA_CHUNK", "MFA_DFA_ARENA", "MFA_SET_SPLIT",
         "MFA_SET_SPLIT_ROUNDS", "MFA_SET_SPLIT_LOOKBACK", "DIPLOMA_PIECE_BYTES")
REGEX_IMAGES = ("k_512", "k_512_rev", "k_1024", "k_2048", "deep")
RAW_NODES = (257, 1025, 2048)
ZEROS = (0, 0, 0, 0, 0, 0)


@pytest.fixture()
def env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MFA_DFA_SPLIT_MIN", str(SPLIT_MIN))
    monkeypatch.setenv("MFA_DFA_CHUNK", str(CHUNK))
    return monkeypatch


def wave_image(env, blob):
    """created with a low tabulation limit, so it falls over to the set walk by itself -- and, beyond 256 nodes, to the wave kernels"""
    env.setenv("MFA_DFA_STATE_LIMIT", "2")
    img = capi.Image(blob)
    env.delenv("MFA_DFA_STATE_LIMIT")
    assert img.info()["dfa_states"] == 0 and img.info()["n_nodes"] > LANE_MAX_NODES and img.resume_state_bytes() == 4 * WIDE_WORDS
    return img


def forced(env, blob, wave):
    """a narrow image as a set-walk image: of the lane kernel, or with MFA_SET_WAVE=1 of the wave kernels"""
    env.setenv("MFA_NFA_SETWALK", "1")
    if wave:
        env.setenv("MFA_SET_WAVE", "1")
    img = capi.Image(blob)
    env.delenv("MFA_NFA_SETWALK")
    env.delenv("MFA_SET_WAVE", raising=False)
    assert img.info()["dfa_states"] == 0 and img.resume_state_bytes() == (4 * WIDE_WORDS if wave else 48)
    return img


def mismatch(got, want, strings, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d mismatches, first string %d (len %d) want %d got %d" % (what, bad.size, bad[0], len(strings[bad[0]]), want[bad[0]], got[bad[0]])


def ragged_batch(alpha, rng):
    """the lengths of tests/test_nfa_set_split_gpu.py: split_min - 1, split_min, split_min + 1 and around chunk multiples up to 5 KiB, between
    short and empty strings that put them at unaligned offsets"""
    longs = [SPLIT_MIN - 1, SPLIT_MIN, SPLIT_MIN + 1, 17 * CHUNK - 1, 17 * CHUNK, 17 * CHUNK + 1, 32 * CHUNK - 1, 32 * CHUNK, 32 * CHUNK + 1, 3000, 5 * 1024]
    out = []
    for k, ln in enumerate(longs + longs):
        out.append(rnd(alpha, int(rng.integers(0, 40)), rng) if k % 3 else b"")
        out.append(rnd(alpha, ln, rng))
    return out + [b"", rnd(alpha, 7, rng)]


def guarded_match(img, strings, stream=None):
    """one mfa_match_batch call in exactly the room the read rule asks for, with 64 guard bytes on either side of the results: (result
    bytes, host offsets)"""
    import torch
    d_bytes, d_off, off = upload(strings, exact=True)
    n = len(strings)
    res = torch.full((n + 128,), 7, dtype=torch.uint8, device="cuda")
    img.match_tensors(d_bytes, d_off, res[64:64 + n], stream=stream)
    torch.cuda.synchronize()
    return results_of(res, n), off


def check_split_report(img, off, what, arena=ARENA):
    n_long, chunks, chunk = expected_split(off, SPLIT_MIN, CHUNK, arena)
    got = img.last_set_split()
    assert n_long > 0 and chunks > 0 and got[:3] == (n_long, chunks, chunk), (what, got, (n_long, chunks, chunk))
    assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0) and img.last_kernel_ms() > 0.0
    assert img.info()["last_kernel"] == capi.KERNEL_NODESET
    return got


def raw_by_nodes():
    """n_nodes -> (name, blob, strings, want): one image per node count, the directions taking turns"""
    corpus, dropped = raw_corpus_once(RAW_NODES, 2)
    assert dropped == 0
    out = {}
    for k, n_nodes in enumerate(RAW_NODES):
        have = [c for c in corpus if image.blob_info(c[1])["n_nodes"] == n_nodes]
        out[n_nodes] = have[k % 2]
    return out


# ---- answers ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", REGEX_IMAGES)
def test_ragged_batch_regex_images(env, name, tmp_path):
    blob, alphabet, min_len = wide_regex_images(tmp_path)[name]
    rng = np.random.default_rng(91 + len(name))
    strings = ragged_batch(alphabet, rng)
    want = oracle_lib.OracleImage(blob).match(strings)
    if name != "deep":
        assert 0 < int(want.sum()) < len(strings)
    img = wave_image(env, blob)
    got, off = guarded_match(img, strings)
    mismatch(got, want, strings, name)
    assert sum(1 for o, s in zip(off, strings) if len(s) >= SPLIT_MIN and int(o) % 16) > 4      # long strings at unaligned offsets
    check_split_report(img, off, name)


@pytest.mark.parametrize("n_nodes", RAW_NODES)
def test_raw_images_own_long_strings(env, n_nodes):
    """the raw images' own strings of 1024, 1025, 2049 and 4096 bytes are cut, those of 1023 and less are not"""
    name, blob, strings, want = raw_by_nodes()[n_nodes]
    assert {1023, 1024, 1025, 2049} <= {len(s) for s in strings} and max(len(s) for s in strings) <= 5 * 1024
    env.setenv("MFA_NFA_SETWALK", "1")
    img = capi.Image(blob)
    env.delenv("MFA_NFA_SETWALK")
    assert img.info()["n_nodes"] == n_nodes and img.resume_state_bytes() == 4 * WIDE_WORDS
    got, off = guarded_match(img, strings)
    mismatch(got, want, strings, name)
    report = check_split_report(img, off, name)
    assert report[0] == sum(1 for s in strings if len(s) >= SPLIT_MIN) >= 4


def test_all_four_instantiations_are_walked(tmp_path):
    """the images of the two tests above keep their tables behind the stacks in LDS, and read them through L2, in both scan directions.
    The placement is the harness's printed table words and depth, (4 * depth + words) * 4 against 65536"""
    images = wide_regex_images(tmp_path)
    cases = [(name, images[name][0]) for name in REGEX_IMAGES] + [(c[0], c[1]) for c in raw_by_nodes().values()]
    seen = {}
    for name, blob in cases:
        tables = run_wide_pieces(emul_exe("nfa_set_wave_resume"), tmp_path, blob, [[b"ab"]])[0]
        seen.setdefault((image.blob_info(blob)["reversed"], tables_in_lds(tables)), []).append(name)
    assert set(seen) == {(0, True), (0, False), (1, True), (1, False)}, seen


# ---- the resume form ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k_512", "k_512_rev"])
def test_resume_form(env, name, tmp_path):
    """pieces in three rounds, long pieces cut: each round the records equal the whole-walk harness's word for word (guard quarters round
    them) and the results the oracle's; the count of queued pieces is the count of long pieces.  Dead and INVALID records are not queued"""
    emul = emul_exe("nfa_set_wave_resume")
    blob, alphabet, _ = wide_regex_images(tmp_path)[name]
    is_rev = image.blob_info(blob)["reversed"]
    rng = np.random.default_rng(17)
    img = wave_image(env, blob)
    lens = [(1500, 1024, 2000), (40, 3000, 0), (1023, 1025, 64), (0, 5000, 1100), (1100, 1100, 1100), (5, 0, 1024), (2048, 10, 2049)]
    strings = [rnd(alphabet, sum(t), rng) for t in lens]              # (ab on (a|b)*a(a|b)^k: no set dies, every long piece is queued)
    ora = oracle_lib.OracleImage(blob)
    rounds = [[], [], []]
    for s, (a, b, c) in zip(strings, lens):
        n = len(s)
        cuts = [(n - a, n), (n - a - b, n - a), (0, n - a - b)] if is_rev else [(0, a), (a, a + b), (a + b, n)]
        for r in range(3):
            rounds[r].append(cuts[r])
    buf = new_records(len(strings), WIDE_WORDS)
    for r in range(3):
        pieces = pieces_of(strings, rounds[r])
        got = feed_records(img, pieces, buf, WIDE_WORDS)
        seen = [s[rounds[r][k][0]:] if is_rev else s[:rounds[r][k][1]] for k, s in enumerate(strings)]
        mismatch(got, ora.match(seen), seen, "round %d" % r)
        _, _, recs_host = run_wide_pieces(emul, tmp_path, blob, [seen])
        assert np.array_equal(records_of(buf, len(strings), WIDE_WORDS), recs_host), "round %d" % r
        assert img.last_set_split()[0] == sum(1 for p in pieces if len(p) >= SPLIT_MIN) >= 3
        assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)
    # dead, INVALID and a live neighbour, each with a long piece: only the neighbour is queued
    rows = np.stack([record(WIDE_WORDS, LIVE), record(WIDE_WORDS, INVALID), record(WIDE_WORDS, 0)])
    buf = new_records(3, WIDE_WORDS, rows)
    got = feed_records(img, [strings[1]] * 3, buf, WIDE_WORDS)
    recs = records_of(buf, 3, WIDE_WORDS)
    assert list(got[:2]) == [0, 2] and got[2] == ora.match([strings[1]])[0]
    assert list(recs[0]) == [LIVE] + [0] * (WIDE_WORDS - 1) and list(recs[1]) == [INVALID] + [0] * (WIDE_WORDS - 1) and recs[2, 0] == LIVE
    assert img.last_set_split()[0] == 1


def test_resume_form_without_result_bytes(env, tmp_path):
    """d_results == NULL behind queued pieces (the resolve kernel's RESUME form writes the record alone): two rounds of long pieces
    without result bytes, then a short round with them -- the oracle's answers, the whole-walk harness's records"""
    blob, alphabet, _ = wide_regex_images(tmp_path)["k_512_rev"]
    img = wave_image(env, blob)
    rng = np.random.default_rng(23)
    strings = [rnd(alphabet, ln, rng) for ln in (2048 + 1500 + 300, 1024 + 1025 + 7, 5000 + 1024 + 0, 100 + 3000 + 1023)]
    thirds = [(2048, 1500), (1024, 1025), (5000, 1024), (100, 3000)]
    rounds = [[s[len(s) - a:] for s, (a, b) in zip(strings, thirds)], [s[len(s) - a - b:len(s) - a] for s, (a, b) in zip(strings, thirds)],
              [s[:len(s) - a - b] for s, (a, b) in zip(strings, thirds)]]      # (the image scans from the end)
    buf = new_records(len(strings), WIDE_WORDS)
    for r in range(2):
        assert feed_records(img, rounds[r], buf, WIDE_WORDS, results=False) is None
        assert img.last_set_split()[0] == sum(1 for p in rounds[r] if len(p) >= SPLIT_MIN) >= 3
    got = feed_records(img, rounds[2], buf, WIDE_WORDS)
    mismatch(got, oracle_lib.OracleImage(blob).match(strings), strings, "no result bytes")
    _, _, recs_host = run_wide_pieces(emul_exe("nfa_set_wave_resume"), tmp_path, blob, [strings])
    assert np.array_equal(records_of(buf, len(strings), WIDE_WORDS), recs_host)


# ---- counts -----------------------------------------------------------------------------------------------------------------------------
def counts_against_the_harness(env, tmp_path, img, blob, strings, rounds, lookback):
    """one batch of long strings only: the answers are the oracle's and the counts of mfa_last_set_split those of the host harness on the
    same batch with the same settings (it cuts every string, so every string here is long)"""
    assert all(len(s) >= SPLIT_MIN for s in strings)
    env.setenv("MFA_SET_SPLIT_ROUNDS", str(rounds))
    env.setenv("MFA_SET_SPLIT_LOOKBACK", str(lookback))
    got, off = guarded_match(img, strings)
    mismatch(got, oracle_lib.OracleImage(blob).match(strings), strings, "rounds %d" % rounds)
    report = check_split_report(img, off, "rounds %d" % rounds)
    (_, host, _), = run_wave_split(emul_exe("nfa_set_wave_split"), tmp_path, blob, strings, (CHUNK,), (lookback,), (rounds,))
    assert report[3:] == (host["rewalked"], host["serial_strings"], host["serial_bytes"]), (report, host)
    return report, host


def test_counter_is_resolved_serially(env, tmp_path):
    """(a^300)*, 303 nodes: a position modulo 300 cannot be guessed, every long string is resolved serially at 0 and at 3 rounds, and the
    answers are right.  (Lengths are multiples of 16: the chunk grid starts at the string.)"""
    blob = front_end_blob(COUNTER300, tmp_path)
    env.setenv("MFA_DFA_STATE_LIMIT", "100")
    img = capi.Image(blob)
    env.delenv("MFA_DFA_STATE_LIMIT")
    assert img.info()["n_nodes"] == 303 and img.info()["dfa_states"] == 0
    strings = [b"a" * 2400, b"a" * 2416, b"a" * 4800, b"a" * 3008, b"a" * 1600 + b"b" + b"a" * 399, b"a" * 4999]
    assert list(oracle_lib.OracleImage(blob).match(strings)) == [1, 0, 1, 0, 0, 0]
    r0, _ = counts_against_the_harness(env, tmp_path, img, blob, strings, 0, 256)
    r3, _ = counts_against_the_harness(env, tmp_path, img, blob, strings, 3, 256)
    assert r0[3] == 0 and r0[4] == len(strings) and r3[3] > 0 and r3[4] == len(strings) and 0 < r3[5] < r0[5]


def test_literal_prefix_guesses_the_home_set(env, tmp_path):
    """xyz(a|b)*a(a|b)^52: a walk from {start} dies on the text in front of every chunk, the home set's does not; behind a run of z both die
    and the guess is the home set itself.  Nothing of the accepted strings is left to the serial walk"""
    blob = front_end_blob(PREFIX_WIDE, tmp_path)
    img = wave_image(env, blob)
    rng = np.random.default_rng(5)
    body = ab_strings([1500, 2048, 4000], rng, tail=b"a" + b"b" * 52)
    strings = [b"xyz" + s for s in body]
    report, host = counts_against_the_harness(env, tmp_path, img, blob, strings, 0, 64)
    assert report[3:] == (0, 0, 0) and host["home_guesses"] == 0
    strings = strings + [b"xyz" + body[0][:300] + b"z" * 200 + body[0][300:], body[1]]
    for rounds in (0, 3):
        _, host = counts_against_the_harness(env, tmp_path, img, blob, strings, rounds, 64)
        assert host["home_guesses"] > 0


# ---- knobs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob", ["MFA_SET_SPLIT", "MFA_DFA_SPLIT", None], ids=["MFA_SET_SPLIT=0", "MFA_DFA_SPLIT=0", "no long string"])
def test_six_zeros_and_the_same_answers(env, knob, tmp_path):
    blob, alphabet, _ = wide_regex_images(tmp_path)["k_512"]
    img = wave_image(env, blob)
    strings = ragged_batch(alphabet, np.random.default_rng(4))
    want = oracle_lib.OracleImage(blob).match(strings)
    on, _ = guarded_match(img, strings)
    assert img.last_set_split()[0] > 0
    mismatch(on, want, strings, "on")
    if knob is None:
        strings = [s[:SPLIT_MIN - 1] for s in strings]
        want = oracle_lib.OracleImage(blob).match(strings)
    else:
        env.setenv(knob, "0")
    off, _ = guarded_match(img, strings)
    mismatch(off, want, strings, "%s=0" % knob)
    assert img.last_set_split() == ZEROS and img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)
    mismatch(feed_records(img, strings, new_records(len(strings), WIDE_WORDS), WIDE_WORDS), want, strings, "%s=0, resume form" % knob)
    assert img.last_set_split() == ZEROS


def test_arena_shrunk_chunk_grows(env, tmp_path):
    """MFA_DFA_ARENA=16: the plan kernel grows the chunk size so that the chunks stay near 16"""
    blob, alphabet, _ = wide_regex_images(tmp_path)["k_512_rev"]
    img = wave_image(env, blob)
    env.setenv("MFA_DFA_ARENA", "16")
    strings = ragged_batch(alphabet, np.random.default_rng(8))
    got, off = guarded_match(img, strings)
    mismatch(got, oracle_lib.OracleImage(blob).match(strings), strings, "arena 16")
    report = check_split_report(img, off, "arena 16", arena=16)
    assert report[2] > 16 * CHUNK


def test_queue_overflow_and_the_arena_cap(env, tmp_path):
    """16 400 strings of 1 040 bytes on the 259-node image: 16 384 are queued and cut, the rest are walked whole by the waves that were
    refused a slot, all answers are right -- and 17 MB of long strings pass the wave images' arena cap of 32 768 chunks, so the plan
    kernel grows the chunk size from the 64 bytes asked for.  (1 040 is a multiple of 16: every string has the same chunk count,
    whichever 16 384 get the slots.)"""
    blob, alphabet, _ = wide_regex_images(tmp_path)["k_512"]
    img = wave_image(env, blob)
    rng = np.random.default_rng(6)
    kinds = [rnd(alphabet, 1040, rng) for _ in range(16)]
    want16 = oracle_lib.OracleImage(blob).match(kinds)
    assert 0 < int(want16.sum()) < 16
    n, qcap = 16400, 16384
    strings = [kinds[k % 16] for k in range(n)]
    got, off = match_on_gpu(img, strings, exact=True)
    mismatch(got, np.tile(want16, n // 16), strings, "queue overflow")
    n_long, chunks, chunk = expected_split(off[:qcap + 1], SPLIT_MIN, CHUNK, ARENA)
    assert (n_long, chunk) == (qcap, 528) and chunks == 2 * qcap
    assert img.last_set_split()[:3] == (n_long, chunks, chunk)
    assert img.last_dfa_split() == (0, 0, 0) and img.last_dfa_spec() == (0, 0, 0)


@pytest.mark.parametrize("name", ["nfa_abb_thompson", "nfa_star4_ssnf"])
def test_narrow_fixtures_as_wave_images(env, name):
    """MFA_SET_WAVE=1 images are wave images: the lane split's answers byte for byte, and its report word for word (one rule, two paths)"""
    blob = blob_of(name, 0)
    lane, wave = forced(env, blob, False), forced(env, blob, True)
    rng = np.random.default_rng(12)
    strings = ragged_batch(b"ab", rng)
    strings[5] = strings[5][:-3] + b"abb"
    if image.blob_info(blob)["reversed"]:
        strings = [s[::-1] for s in strings]
    want = oracle_lib.OracleImage(blob).match(strings)
    got_lane, _ = match_on_gpu(lane, strings, exact=True)
    got_wave, off = guarded_match(wave, strings)
    assert np.array_equal(got_lane, got_wave)
    mismatch(got_wave, want, strings, name)
    assert check_split_report(wave, off, name) == lane.last_set_split()


# ---- streams, capture, host pointers, mixed objects -----------------------------------------------------------------------------------------
def test_non_default_stream(env, tmp_path):
    import torch
    blob, alphabet, _ = wide_regex_images(tmp_path)["k_512"]
    img = wave_image(env, blob)
    strings = ragged_batch(alphabet, np.random.default_rng(33))
    s = torch.cuda.Stream()
    got, off = guarded_match(img, strings, stream=s)
    mismatch(got, oracle_lib.OracleImage(blob).match(strings), strings, "stream")
    check_split_report(img, off, "stream")


def test_call_is_capturable(env, tmp_path):
    """after a first uncaptured call, one call is captured on one stream (the chain is linear) and replayed with new bytes in the same buffers"""
    import torch
    blob, alphabet, _ = wide_regex_images(tmp_path)["k_512"]
    img = wave_image(env, blob)
    rng = np.random.default_rng(13)
    first = [rnd(alphabet, 3000, rng), b"ab", rnd(alphabet, 1024, rng), b"abb", b""]
    second = [rnd(alphabet, len(s), rng) for s in first]
    ora = oracle_lib.OracleImage(blob)
    assert not np.array_equal(ora.match(first), ora.match(second))
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


def test_host_pointers(env, tmp_path):
    """mfa_match_batch_host and mfa_match_batch_resume_set_wide_host cut long strings as the device calls do"""
    blob, alphabet, _ = wide_regex_images(tmp_path)["k_512_rev"]
    img = wave_image(env, blob)
    strings = ragged_batch(alphabet, np.random.default_rng(14))
    want = oracle_lib.OracleImage(blob).match(strings)
    data, off = oracle_lib.pack(strings)
    data = np.concatenate([data, np.zeros(16, np.uint8)])
    mismatch(img.match_host(data, off), want, strings, "host")
    n_long = sum(1 for s in strings if len(s) >= SPLIT_MIN)
    assert img.last_set_split()[0] == n_long
    states = np.zeros(len(strings) * WIDE_WORDS, dtype=np.uint32)
    mismatch(img.match_host_resume_set_wide(data, off, states), want, strings, "host, resume form")
    assert img.last_set_split()[0] == n_long and (states.reshape(-1, WIDE_WORDS)[:, 0] == LIVE).all()


def test_mixed_object_inherits_the_path(env, tmp_path):
    """a mixed object whose wave segment holds long strings answers what the per-image calls answer"""
    blob_w, alphabet, _ = wide_regex_images(tmp_path)["k_512"]
    blob_t = blob_of("nfa_star4_ssnf", 0)
    wave, tab = wave_image(env, blob_w), capi.Image(blob_t)
    assert tab.info()["dfa_states"] != 0
    rng = np.random.default_rng(21)
    segments = [ragged_batch(alphabet, rng), [b"ab" * 40 + b"a", b"c" * 2000 + b"a", b"", b"abab" * 300 + b"a"]]
    mixed = capi.Mixed([wave, tab])
    got = mixed_match(mixed, segments)
    mixed.close()
    want = np.concatenate([oracle_lib.OracleImage(b).match(seg) for b, seg in zip((blob_w, blob_t), segments)])
    mismatch(got, want, segments[0] + segments[1], "mixed")
    assert wave.last_set_split()[0] == sum(1 for s in segments[0] if len(s) >= SPLIT_MIN)
    own = np.concatenate([match_on_gpu(wave, segments[0])[0], match_on_gpu(tab, segments[1])[0]])
    assert np.array_equal(got, own)


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def counter_cli(tmp_path, words, extra_env):
    p = subprocess.run([DIPLOMA, "-dump"], input=COUNTER300 + "\n", capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    blob = image.blob_from_dump(p.stdout)
    assert image.blob_info(blob)["n_nodes"] > LANE_MAX_NODES
    want = [int(x) for x in oracle_lib.OracleImage(blob).match([w.encode() for w in words])]
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(MFA_DFA_STATE_LIMIT="100", MFA_VERBOSE="1", MFA_DFA_SPLIT_MIN=str(SPLIT_MIN), MFA_DFA_CHUNK=str(CHUNK), **extra_env)
    r = subprocess.run([DIPLOMA, "-match"], input=COUNTER300 + "\n" + "\n".join(words) + "\nexit\n", capture_output=True, text=True, cwd=tmp_path, env=e)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in r.stdout.split() if x in ("0", "1")] == want
    return want, r.stderr, blob


def counter_image(env, blob):
    """the image `diploma -match` makes of (a^300)* under the limit counter_cli sets"""
    env.setenv("MFA_DFA_STATE_LIMIT", "100")
    img = capi.Image(blob)
    env.delenv("MFA_DFA_STATE_LIMIT")
    assert img.info()["dfa_states"] == 0 and img.resume_state_bytes() == 4 * WIDE_WORDS
    return img


def test_command_line_long_line(env, tmp_path):
    """`diploma -match` on (a^300)* with lines of 3 000 bytes under MFA_DFA_SPLIT_MIN=1024: cut, resolved serially, the oracle's answers;
    the message keeps naming the main kernel"""
    words = ["a" * 3000, "a" * 2999, "a" * 300, "a" * 1500 + "b" + "a" * 1499]
    want, err, blob = counter_cli(tmp_path, words, {})
    assert want == [1, 0, 1, 0] and "nfa_set_wave_kernel" in err and "nfa_set_wave_resume_kernel" not in err
    # the command line shows no count: the call it makes for these lines (the host call, under the knobs it ran with) queues the three long ones
    img = counter_image(env, blob)
    data, off = oracle_lib.pack([w.encode() for w in words])
    assert list(img.match_host(np.concatenate([data, np.zeros(16, np.uint8)]), off)) == want
    report = img.last_set_split()
    assert report[0] == 3 and report[2] == CHUNK and report[4] == 3      # ... and the counter resolves each of them serially


def test_command_line_pieces_that_are_cut(env, tmp_path):
    """DIPLOMA_PIECE_BYTES=2048 with strings of 5 000 bytes: match_in_pieces feeds pieces of 2 048 bytes through the wide call, and every
    such piece is itself cut"""
    words = ["a" * 5000, "a" * 4800, "a" * 2400 + "b" + "a" * 2399, "a" * 600]
    want, err, blob = counter_cli(tmp_path, words, {"DIPLOMA_PIECE_BYTES": "2048"})
    assert want == [0, 1, 0, 1] and "nfa_set_wave_resume_kernel" in err
    # the command line shows no count: the calls match_in_pieces makes for the three long strings (pieces of 2 048 bytes and the rest through
    # the wide host call, no result bytes before the last), under the knobs it ran with -- every piece that enters alive is queued and cut
    img = counter_image(env, blob)
    strings = [w.encode() for w in words[:3]]
    states = np.zeros(len(strings) * WIDE_WORDS, dtype=np.uint32)
    queued = []
    for r in range(3):
        data, off = oracle_lib.pack([s[2048 * r:2048 * (r + 1)] for s in strings])
        got = img.match_host_resume_set_wide(np.concatenate([data, np.zeros(16, np.uint8)]), off, states, want_results=r == 2)
        queued.append(img.last_set_split()[0])
    assert list(got) == want[:3]
    assert queued == [3, 3, 0]                       # (the last pieces are 904, 704 and 704 bytes; the string with the b is still alive in round 1: the b is byte 2400)
