"""Long strings of wave images cut across the GPU, the part that can be wrong without one (csrc/nfa_set_wave_split_core.h: the wide chunk
records, the guess from two seeds, the waves of round 0 and of a repair round, the resolve loop over records, the hand-over of the resume
kernel; csrc/image_host.cpp: the wide home set), compiled for the host (tests/emul/nfa_set_wave_split_emul.cpp) and run one wave at a
time in the kernels' order.  Inside the harness the final record of every string is compared, word for word, with nfa_wave_walk_from over
the whole string; here the result bytes are compared with the CPU restatement, and on the narrow fixtures the counts with those of the
lane path's harness (tests/emul/nfa_set_split_emul.cpp).  The kernels around it are checked by tests/test_nfa_set_wave_split_gpu.py."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib
from mfa_amd import image
from setwalk_lib import (CHUNKS, COUNTER300, COUNT_KEYS, EDGE_LENGTHS, INVALID, LIVE, LOOKBACKS, PREFIX_WIDE, REPAIR_ROUNDS, START, WIDE_WORDS, ab_strings, check_records_are_clean,
                         chunk_lengths, fixture_corpus, pack_every_offset, pieces_of, raw_corpus_once, record, run_lane_split, run_wave_split, run_wide_pieces,
                         run_wide_split_pieces, wide_regex_images, words_of)
from testlib import NFA_NAMES, emul_exe, front_end_blob, out_offsets

REGEX_IMAGES = ("k_512", "k_512_rev", "k_1024", "k_2048", "deep")
RAW = ((257, 1025, 2048), 2)
SPLIT_LENGTHS = chunk_lengths() + EDGE_LENGTHS      # around multiples of every chunk size, and 1023, 1024, 1025, 2049


@pytest.fixture(scope="module")
def emul():
    return emul_exe("nfa_set_wave_split")


def check_all(runs, want, strings, what, n_nodes):
    assert len(runs) == len(CHUNKS) * len(LOOKBACKS) * len(REPAIR_ROUNDS)
    for (chunk, lookback, rounds), got, res in runs:
        bad = np.nonzero(res != want)[0]
        assert bad.size == 0, "%s chunk %d lookback %d rounds %d: %d mismatches, first len %d want %d" % (
            what, chunk, lookback, rounds, bad.size, len(strings[bad[0]]), want[bad[0]])
        assert got["checks"] == len(strings) and got["home_nodes"] > 0 and got["W"] == words_of(n_nodes) and got["invalid_ends"] == 0
        if rounds == 0:
            assert got["rewalked"] == 0


def split_strings(pick):
    """one string of every length of SPLIT_LENGTHS, and fillers until, packed back to back, a string's first byte lies at every offset mod 16"""
    strings = pack_every_offset([pick(ln) for ln in SPLIT_LENGTHS], lambda k: pick(1 + k % 7))
    assert {o % 16 for o in out_offsets(strings)} == set(range(16))
    return strings


@pytest.mark.parametrize("name", REGEX_IMAGES)
def test_wide_regex_images(emul, name, tmp_path):
    """259 to 2048 nodes, both directions (k_512_rev and deep scan from the end), chunks of 16 / 32 / 64 bytes, lookback 0 / 8 / 256,
    0 / 1 / 3 / 8 repair rounds"""
    blob, alphabet, min_len = wide_regex_images(tmp_path)[name]
    rng = np.random.default_rng(len(name))
    strings = split_strings(lambda ln: bytes(rng.choice(list(alphabet), size=int(ln)).tolist()))
    want = oracle_lib.OracleImage(blob).match(strings)
    assert 0 < int(want.sum()) < len(strings)
    check_all(run_wave_split(emul, tmp_path, blob, strings, CHUNKS, LOOKBACKS, REPAIR_ROUNDS), want, strings, name, image.blob_info(blob)["n_nodes"])


def test_raw_images(emul, tmp_path):
    """random automata of 257, 1025 and 2048 nodes with their own strings (1023, 1024, 1025, 2049 and 4096 bytes among them), both
    directions; the six harness runs side by side (each is one process and takes most of a minute)"""
    corpus, dropped = raw_corpus_once(*RAW)
    assert dropped == 0 and len(corpus) == 6
    assert {image.blob_info(c[1])["reversed"] for c in corpus} == {0, 1}

    def one(case):
        name, blob, strings, want = case
        assert set(EDGE_LENGTHS) <= {len(s) for s in strings}
        folder = tmp_path / name
        folder.mkdir()
        return run_wave_split(emul, folder, blob, strings, CHUNKS, LOOKBACKS, REPAIR_ROUNDS)

    with ThreadPoolExecutor(max_workers=max(1, min(len(corpus), os.cpu_count() or 1))) as pool:
        all_runs = list(pool.map(one, corpus))
    for (name, blob, strings, want), runs in zip(corpus, all_runs):
        check_all(runs, want, strings, name, image.blob_info(blob)["n_nodes"])


@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reversed"])
@pytest.mark.parametrize("name", NFA_NAMES)
def test_narrow_fixtures_count_what_the_lane_path_counts(emul, name, rev, tmp_path):
    """every memory-less fixture through wave tables: the answers are the oracle's, and the chunks walked again, the strings resolved
    serially and their bytes are those of nfa_set_split_emul on the same strings, chunks, lookback and rounds -- both paths state the
    same rule, so a difference is a bug in one of them"""
    blob, strings = fixture_corpus(name, rev)
    assert {o % 16 for o in out_offsets(strings)} == set(range(16))
    want = oracle_lib.OracleImage(blob).match(strings)
    wave = run_wave_split(emul, tmp_path, blob, strings, CHUNKS, LOOKBACKS, REPAIR_ROUNDS)
    check_all(wave, want, strings, "%s rev %d" % (name, rev), image.blob_info(blob)["n_nodes"])
    lane = run_lane_split(emul_exe("nfa_set_split"), tmp_path, blob, strings, CHUNKS, LOOKBACKS, REPAIR_ROUNDS)
    for (combo, got_w, res_w), (combo_l, got_l, res_l) in zip(wave, lane):
        assert combo == combo_l and np.array_equal(res_w, res_l)
        assert [got_w[k] for k in COUNT_KEYS + ("home_guesses", "home_nodes")] == [got_l[k] for k in COUNT_KEYS + ("home_guesses", "home_nodes")], (name, combo)


# ---- pathologies: slow, never wrong ---------------------------------------------------------------------------------------------------------
def test_counter_is_resolved_serially(emul, tmp_path):
    """(a^300)*, 303 nodes: the set is a position modulo 300 and never converges.  Every long string is resolved serially, without a repair
    round and with three; more rounds leave less to walk; the answers are right"""
    blob = front_end_blob(COUNTER300, tmp_path)
    assert image.blob_info(blob)["n_nodes"] == 303
    strings = [b"a" * ln for ln in (1200, 1500, 1800, 2047, 2400)] + [b"a" * 600 + b"b" + b"a" * 600]
    want = oracle_lib.OracleImage(blob).match(strings)
    assert list(want) == [1, 1, 1, 0, 1, 0]
    (_, got0, res0), (_, got3, res3) = run_wave_split(emul, tmp_path, blob, strings, (64,), (8,), (0, 3))
    assert np.array_equal(res0, want) and np.array_equal(res3, want)
    assert got0["W"] == 10 and got0["serial_strings"] == len(strings) and got3["serial_strings"] == len(strings)
    assert got3["rewalked"] > 0 and 0 < got3["serial_bytes"] < got0["serial_bytes"]


def test_literal_prefix_guesses_the_home_set(emul, tmp_path):
    """xyz(a|b)*a(a|b)^52, 272 nodes: on the text in front of a chunk a walk from {start} dies (no x), and with 64 bytes of lookback the
    home set's walk lives and fixes the set -- but on text that kills the home set's walk too (a run of z, longer than a chunk and its
    lookback), the guess is the home set itself"""
    blob = front_end_blob(PREFIX_WIDE, tmp_path)
    assert image.blob_info(blob)["n_nodes"] > 256
    rng = np.random.default_rng(5)
    body = ab_strings([500, 640, 1000], rng, tail=b"a" + b"b" * 52)
    strings = [b"xyz" + s for s in body] + [b"xyz" + body[0][:100] + b"z" * 200 + body[0][100:], body[1]]
    want = oracle_lib.OracleImage(blob).match(strings)
    assert list(want) == [1, 1, 1, 0, 0]
    runs = run_wave_split(emul, tmp_path, blob, strings, (64,), (64, 256), (0, 3))
    for _, got, res in runs:
        assert np.array_equal(res, want) and got["checks"] == len(strings)
        assert got["home_guesses"] > 0                # string 3 holds 200 z: chunks begin behind 64 of them, and both seeds die on those
    # the home set lies inside the loop: 64 bytes in front of a chunk fix the set, and nothing of the accepted strings is left to the serial walk
    (_, three, _), = run_wave_split(emul, tmp_path, blob, strings[:3], (64,), (64,), (0,))
    assert (three["serial_strings"], three["rewalked"], three["home_guesses"]) == (0, 0, 0)


def test_k_512_needs_no_repair(emul, tmp_path):
    """(a|b)*a(a|b)^50 (259 nodes) with lookback 256 and 64-byte chunks on random ab: the last 51 bytes fix the set, so every guess is right --
    0 chunks walked again, 0 strings resolved serially, in both directions"""
    images = wide_regex_images(tmp_path)
    assert images["k_512"][2] < 64
    strings = ab_strings([1024, 1025, 2048, 3000, 5 * 1024, 63, 64, 65], np.random.default_rng(50))
    for name in ("k_512", "k_512_rev"):
        blob = images[name][0]
        want = oracle_lib.OracleImage(blob).match(strings)
        assert 0 < int(want.sum()) < len(strings)
        for _, got, res in run_wave_split(emul, tmp_path, blob, strings, (64,), (256,), (0, 3)):
            assert np.array_equal(res, want)
            assert (got["rewalked"], got["serial_strings"], got["serial_bytes"]) == (0, 0, 0)


def test_overflowing_chunk_is_resolved_around(emul, tmp_path):
    """xyz(a|b)*c(DEEP)* with DEEP ten nested alternations: the home set lies inside DEEP, whose epsilon chains need a deep stack, and the
    strings -- xyz, a run of a and b, at most one c at the end -- never get there.  With the stacks cut to the fewest slots at which the
    whole walk of these strings still finishes, the chunks walked from the home set (a walk from {start} dies in mid-text) overflow and end
    INVALID; the string is resolved around them, and the final record is the whole walk's (the harness holds it to that)"""
    deep = "a"
    for _ in range(10):
        deep = "((" + deep + "|b)|c)"
    blob = front_end_blob("xyz(a|b)*c(" + deep + ")*", tmp_path)
    rng = np.random.default_rng(3)
    strings = [b"xyz" + s for s in ab_strings([300, 500, 640], rng)]
    strings = [strings[0] + b"c", strings[1], strings[2] + b"c"]
    want = oracle_lib.OracleImage(blob).match(strings)
    assert list(want) == [1, 0, 1]
    (_, got, res), = run_wave_split(emul, tmp_path, blob, strings, (64,), (8,), (0,), depth=0)
    assert list(res) == [2, 2, 2]                                           # no slot at all: the whole walk overflows too, and the records say so
    depth = next(d for d in range(1, 12) if 2 not in run_wave_split(emul, tmp_path, blob, strings, (64,), (8,), (0,), depth=d)[0][2])
    (_, got0, res0), (_, got3, res3) = run_wave_split(emul, tmp_path, blob, strings, (64,), (8,), (0, 3), depth=depth)
    assert np.array_equal(res0, want) and np.array_equal(res3, want)
    assert got0["invalid_ends"] > 0 and got0["serial_strings"] == len(strings) and got0["home_guesses"] > 0
    assert got3["rewalked"] > 0 and got3["serial_bytes"] < got0["serial_bytes"]
    # with the stacks the tables ask for nothing overflows
    for _, got, res in run_wave_split(emul, tmp_path, blob, strings, (64,), (8,), (0, 3)):
        assert np.array_equal(res, want) and got["invalid_ends"] == 0


# ---- the resume form ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k_512", "k_512_rev"])
def test_resume_form_pieces_equal_the_whole_walk(emul, name, tmp_path):
    """pieces in three rounds with a split minimum of 200 bytes: pieces of 200 bytes and more that enter with a live set are queued and
    cut, the others are walked whole; each round's answers are the oracle's on what was given so far and the final records are, word
    for word, those of the whole-walk harness (tests/emul/nfa_set_wave_resume_emul.cpp) on the whole strings"""
    blob, alphabet, min_len = wide_regex_images(tmp_path)[name]
    is_rev = image.blob_info(blob)["reversed"]
    rng = np.random.default_rng(17)
    lens = [(300, 200, 450), (40, 700, 0), (199, 201, 64), (0, 1025, 230), (230, 230, 230), (5, 0, 200), (512, 10, 513)]
    strings = [bytes(rng.choice(list(alphabet), size=sum(t)).tolist()) for t in lens]
    rounds = [[], [], []]
    for s, (a, b, c) in zip(strings, lens):
        n = len(s)
        cuts = [(n - a, n), (n - a - b, n - a), (0, n - a - b)] if is_rev else [(0, a), (a, a + b), (a + b, n)]
        for r in range(3):
            rounds[r].append(cuts[r])
    ora = oracle_lib.OracleImage(blob)
    digits, queued, recs = run_wide_split_pieces(emul, tmp_path, blob, [pieces_of(strings, row) for row in rounds], 64, 64, 3, 200)
    assert queued == [sum(1 for t in lens if t[r] >= 200) for r in range(3)] and min(queued) >= 3
    for r in range(3):
        seen = [s[rounds[r][k][0]:] if is_rev else s[:rounds[r][k][1]] for k, s in enumerate(strings)]
        assert np.array_equal(digits[r], ora.match(seen)), "round %d" % r
    _, whole_digits, whole_recs = run_wide_pieces(emul_exe("nfa_set_wave_resume"), tmp_path, blob, [strings])
    assert np.array_equal(recs, whole_recs) and np.array_equal(digits[2], whole_digits[0])
    check_records_are_clean(recs, image.blob_info(blob)["n_nodes"], WIDE_WORDS)


def test_resume_form_queues_live_records_only(emul, tmp_path):
    """dead, INVALID, a record of a tag nobody writes, one with a node the image lacks, and a live neighbour, each with a long piece:
    only the neighbour is queued, the others keep their answers and their records"""
    blob, alphabet, _ = wide_regex_images(tmp_path)["k_512"]
    rng = np.random.default_rng(4)
    piece = bytes(rng.choice(list(alphabet), size=600).tolist())
    rows = np.stack([record(WIDE_WORDS, LIVE), record(WIDE_WORDS, INVALID), record(WIDE_WORDS, 7), record(WIDE_WORDS, LIVE, {63: 1 << 31}), record(WIDE_WORDS, START)])
    digits, queued, recs = run_wide_split_pieces(emul, tmp_path, blob, [[piece] * len(rows)], 64, 64, 3, 200, states=rows)
    assert queued == [1]
    assert list(digits[0]) == [0, 2, 2, 2, oracle_lib.OracleImage(blob).match([piece])[0]]
    assert list(recs[0]) == [LIVE] + [0] * (WIDE_WORDS - 1)
    for k in (1, 2, 3):
        assert list(recs[k]) == [INVALID] + [0] * (WIDE_WORDS - 1)
    assert recs[4, 0] == LIVE and recs[4, 4:].any()
    # a second piece on the live record it left: queued again, from a set that is not {start}
    digits2, queued2, recs2 = run_wide_split_pieces(emul, tmp_path, blob, [[piece] * len(rows)], 64, 64, 0, 200, states=recs)
    assert queued2 == [1] and digits2[0][4] == oracle_lib.OracleImage(blob).match([piece + piece])[0] and list(digits2[0][:4]) == [0, 2, 2, 2]


def test_harness_under_sanitizers(tmp_path):
    """the harness once more with -fsanitize=address,undefined, a stand-alone program, on one image: k_512 scanning from the end, in the
    room the read rule gives and not a byte more, with the stacks and the records at exactly their sizes; the split form and the resume
    form"""
    exe = emul_exe("nfa_set_wave_split", "-fsanitize=address,undefined -fno-sanitize-recover=all")
    blob, alphabet, _ = wide_regex_images(tmp_path)["k_512_rev"]
    rng = np.random.default_rng(9)
    pick = lambda ln: bytes(rng.choice(list(alphabet), size=int(ln)).tolist())
    strings = pack_every_offset([pick(ln) for ln in (0, 1, 15, 16, 17, 63, 64, 65, 129, 700, 1025)], lambda k: pick(1 + k % 7))
    want = oracle_lib.OracleImage(blob).match(strings)
    for (chunk, lookback, rounds), got, res in run_wave_split(exe, tmp_path, blob, strings, (16, 64), (0, 8, 256), (0, 3)):
        assert np.array_equal(res, want) and got["checks"] == len(strings)
    pieces = [[pick(300), pick(17), b""], [pick(64), pick(500), pick(200)]]
    digits, queued, _ = run_wide_split_pieces(exe, tmp_path, blob, pieces, 32, 8, 1, 200)
    assert queued == [1, 2]
    assert np.array_equal(digits[1], oracle_lib.OracleImage(blob).match([b + a for a, b in zip(*pieces)]))
